"""The fabric all-sources table at world 1 with its rows gathered as uint32
(SPF_F_NEXTHOPS | SPF_T_GATHER_ROWS) against gathered as 8-bit level rows
(SPF_F_NEXTHOPS | SPF_T_GATHER_LEVELS): what the copy into the own rank slot
costs in each form (the exchange itself is a no-op on one rank).

Variants alternate in rounds, each round one fresh process per variant on the
same box; per variant the medians over the rounds of
  step_ms    host wall time of one step in a pipelined loop (run x steps, one
             sync: bench.py's _timed_table),
  sync_ms    host wall time of one step that is synchronised (and, for the
             levels form, resolved: one 16-byte trailer read) every time,
  compute_ms / gather_ms   spf_table_elapsed_ms of the last step,
plus gathered_bytes and the form.  --parent-lib PATH adds the variant
"rows_parent": the GATHER_ROWS step of another build of the engine (the
parent commit's libopenr_spf.so), the yardstick of the same box.

  python profiles/table_levels_probe.py [--rounds 5] [--steps 30] [--parent-lib PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(variant, steps, warmup):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from openr_amd import abi
    from openr_amd import topologies as TP

    torch.cuda.init()
    csr = TP.fabric(10000).csr()
    V = csr.num_nodes
    levels = variant == "levels"
    gather = abi.SPF_T_GATHER_LEVELS if levels else abi.SPF_T_GATHER_ROWS
    c = abi.Cluster([0])
    t = abi.Table(c, csr, np.arange(V, dtype=np.uint32), abi.SPF_F_NEXTHOPS | gather)
    for _ in range(warmup):
        t.run()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        t.run(sync=False)
    t.sync()
    step_ms = (time.perf_counter() - t0) * 1e3 / steps
    per = []
    for _ in range(steps):
        t0 = time.perf_counter()
        t.run()
        per.append((time.perf_counter() - t0) * 1e3)
    compute_ms, gather_ms = t.elapsed_ms()
    out = {"variant": variant, "V": V, "plan": t.kernel(0), "step_ms": step_ms,
           "sync_ms": statistics.median(per), "compute_ms": compute_ms, "gather_ms": gather_ms}
    if hasattr(abi.load(), "spf_table_row_form"):  # (an older build lacks it)
        form, scale, gathered = t.row_form()
        out.update(form=form, scale=scale, gathered_bytes=gathered)
        if levels:
            # the rows a consumer expands equal the owner's, all of them
            lo = 0
            while lo < V:
                m = min(1024, V - lo)
                assert (t.expand_rows(lo, m) == t.fetch_rows(lo, m)).all(), lo
                lo += m
            out["expand_equals_owner_rows"] = True
    else:
        out.update(form="rows32", gathered_bytes=V * V * 4)
    t.close()
    c.close()
    print("PROBE " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--child", default=None)
    args = ap.parse_args()
    if args.child:
        return child(args.child, args.steps, args.warmup)
    variants = [("rows", None), ("levels", None)]
    if args.parent_lib:
        variants.insert(0, ("rows_parent", os.path.abspath(args.parent_lib)))
    runs = {name: [] for name, _ in variants}
    for _ in range(args.rounds):
        for name, lib in variants:
            env = dict(os.environ)
            if lib:
                env["OPENR_SPF_LIB"] = lib
            cmd = [sys.executable, os.path.abspath(__file__), "--child", name.split("_")[0],
                   "--steps", str(args.steps), "--warmup", str(args.warmup)]
            p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                # a failed child ends the probe: nothing more is started on the device
                sys.stderr.write(p.stdout + p.stderr)
                raise SystemExit(f"{name}: child exited {p.returncode}")
            line = [l for l in p.stdout.splitlines() if l.startswith("PROBE ")][-1]
            runs[name].append(json.loads(line[6:]))
    out = {}
    for name, rs in runs.items():
        o = {k: rs[-1][k] for k in ("V", "plan", "form", "gathered_bytes") if k in rs[-1]}
        for k in ("step_ms", "sync_ms", "compute_ms", "gather_ms"):
            xs = [r[k] for r in rs]
            o[k] = {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4),
                    "max": round(max(xs), 4)}
        out[name] = o
    print(json.dumps({"rounds": args.rounds, "steps": args.steps, "variants": out}, indent=1))


if __name__ == "__main__":
    main()
