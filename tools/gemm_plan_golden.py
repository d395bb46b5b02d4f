"""From a kernel trace of `gemm_plan_sweep.py --launch` to the golden table of kx_gemm's kernel choice.

    rocprofv3 --kernel-trace -f csv -d DIR -o trace -- python tools/gemm_plan_sweep.py --launch --order-out DIR/order.jsonl
    python tools/gemm_plan_golden.py DIR/trace_kernel_trace.csv DIR/order.jsonl DIR/trace_agent_info.csv --commit REV
    python tools/gemm_plan_golden.py --args-out FILE [--cus N]      # the planner's inputs, for tools/gemm_plan_main.cpp

tests/golden/gemm_plan.json: "launches" is the list of distinct launches, each written as kx_gemm_describe writes a line —
`template<arguments> grid=XxY block=B lds=BYTES`, grid in workgroups, LDS static + dynamic as the trace reports it; "cases" maps a
case name to the indices of its launches in order, or to the refusal's text.  The weight-streaming launches (tile 16) and the
finalize kernel are recorded by family name only: their variant choice is not the planner's.  The file also records the CU count
of the traced device and the commit the trace was taken at.  --args-out writes per case `name|cus|key=value,...|word:hex ...`
with the non-zero 32-bit words of kx_gemm_args.
"""
from __future__ import annotations

import argparse
import csv
import json
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tools"))

SEPARATOR = "sin_kernel"
FAMILY_ONLY = (("gemv_fused_kernel", "gemv_fused"), ("row_stats_finalize_kernel", "kx_row_stats_finalize"))
LIBRARY = ("gemm_kernel", "splitk_reduce_kernel", "splitk_reduce_rows_kernel")


def launch_of(row):
    """One trace row -> a launch record, or None for a kernel that is not the GEMM library's."""
    name = row["Kernel_Name"]
    for needle, family in FAMILY_ONLY:
        if needle in name:
            return {"kernel": family}
    m = re.search(r"\(anonymous namespace\)::(\w+)<(.*)>\(GemmParams\)", name)
    if m is None or not m.group(1).startswith(LIBRARY):
        return None
    args = [a.strip().replace("unsigned short", "bf16_t") for a in m.group(2).split(",")]
    wg = [int(row[f"Workgroup_Size_{d}"]) for d in "XYZ"]
    grid = [int(row[f"Grid_Size_{d}"]) // w for d, w in zip("XYZ", wg)]
    assert grid[2] == 1 and wg[1] == wg[2] == 1, row
    return {"kernel": m.group(1), "args": args, "grid": grid[:2], "block": wg[0], "lds": int(row["LDS_Block_Size"])}


def cases_of(trace_csv, order_jsonl):
    rows = sorted(csv.DictReader(open(trace_csv)), key=lambda r: int(r["Dispatch_Id"]))
    order = [json.loads(line) for line in open(order_jsonl) if line.strip()]
    order = [o for o in order if not o["name"].startswith("<")]
    groups, cur = [], None
    for r in rows:
        if SEPARATOR in r["Kernel_Name"]:
            cur = []
            groups.append(cur)
        elif cur is not None:
            rec = launch_of(r)
            if rec is not None:
                cur.append(rec)
    assert len(groups) == len(order) + 1 and not groups[-1], (len(groups), len(order))
    out = []
    for o, launches in zip(order, groups):
        rec = {"name": o["name"], "launches": launches}
        if o["status"] != "ok":
            assert not launches, o
            rec["refused"] = o["status"].split("kx_gemm: ", 1)[-1]
        out.append(rec)
    return out


def cu_count(agent_csv):
    for r in csv.DictReader(open(agent_csv)):
        if r.get("Agent_Type", "").upper() == "GPU" or r.get("Name", "").startswith("gfx"):
            for key in ("Cu_Count", "Compute_Unit", "Num_Cu"):
                if r.get(key):
                    return int(r[key])
    raise SystemExit("no GPU agent with a CU count in " + agent_csv)


def args_lines(cus):
    """The planner's inputs per case: the sweep's own kx_gemm_args with one fake aligned address for every buffer."""
    import ctypes as C
    sys.path.insert(0, str(ROOT / "kosmos-x_amd"))
    from kosmosx import _hip as H
    import gemm_plan_sweep as S
    for c in S.all_cases():
        g = S.gemm_args(c, H, lambda role, nbytes: 1 << 20)
        words = (C.c_uint32 * (C.sizeof(g) // 4)).from_buffer_copy(g)
        tun = ",".join(f"{k}={v}" for k, v in c.get("tuning", {}).items())
        yield f"{c['name']}|{cus}|{tun}|" + " ".join(f"{i}:{w:x}" for i, w in enumerate(words) if w)


def line_of(rec):
    if "args" not in rec:
        return rec["kernel"]
    return f"{rec['kernel']}<{', '.join(rec['args'])}> grid={rec['grid'][0]}x{rec['grid'][1]} block={rec['block']} lds={rec['lds']}"


def compact(commit, cus, cases):
    table, index, out = [], {}, {}
    for c in cases:
        if "refused" in c:
            out[c["name"]] = "refused: " + c["refused"]
            continue
        ids = []
        for rec in c["launches"]:
            text = line_of(rec)
            if text not in index:
                index[text] = len(table)
                table.append(text)
            ids.append(index[text])
        out[c["name"]] = ids
    lines, cur = [], ""
    for name, v in out.items():                  # several cases per line: the table is data, not prose
        item = json.dumps(name) + ":" + json.dumps(v, separators=(",", ":"))
        if cur and len(cur) + len(item) > 180:
            lines.append(cur)
            cur = ""
        cur += ("," if cur else "") + item
    lines.append(cur)
    head = json.dumps({"commit": commit, "cu_count": cus})[:-1]
    return (head + ',\n"launches":[\n' + ",\n".join(json.dumps(t) for t in table) + '],\n"cases":{\n' + ",\n".join(lines) + "}}\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("trace", nargs="*", help="trace_kernel_trace.csv order.jsonl trace_agent_info.csv")
    ap.add_argument("--commit", default="")
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "gemm_plan.json"))
    ap.add_argument("--args-out", default="")
    ap.add_argument("--cus", type=int, default=256)
    a = ap.parse_args()
    if a.trace:
        trace_csv, order_jsonl, agent_csv = a.trace
        cus = cu_count(agent_csv)
        cases = cases_of(trace_csv, order_jsonl)
        Path(a.out).write_text(compact(a.commit, cus, cases))
        print(f"{a.out}: {len(cases)} cases at {cus} CUs, commit {a.commit}")
    if a.args_out:
        Path(a.args_out).write_text("\n".join(args_lines(a.cus)) + "\n")
        print(a.args_out)
