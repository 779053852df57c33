#!/usr/bin/env python
"""Writes tests/golden/engine_op_trace.json: per case of tests/op_trace_util.py the number of backend calls the plan executor
makes, their histogram by method, the sha256 of the trace text and the peak of live bytes among the tensors the backend
returned.  tests/test_engine_trace_cpu.py recomputes them on the current tree.

The fixture pins the executor's behaviour, so it is regenerated only by a change that MEANS to alter the sequence of backend
calls — and written from the commit before a restructuring, in a checkout of that commit with this tool and the util copied in.

  --dump DIR   also write each case's full trace text as DIR/<case>.txt (for diffing when a hash differs)
  --values     each line also carries exact checksums of every tensor argument and result, and DIR/<case>.results.txt the
               sha256 of every final output and parameter gradient: compare two trees on ONE machine with one thread count
  --out FILE   where to write the JSON (with --values nothing is written unless --out is given)
"""
import argparse
import hashlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--values", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("cases", nargs="*")
    args = ap.parse_args()
    from op_trace_util import BRANCHES, CASES, run_case
    out, reached_all = {}, set()
    for name in (args.cases or CASES):
        t0 = time.time()
        be, results, reached = run_case(name, values=args.values)
        out[name] = be.summary()
        reached_all.update(reached)
        missing = [b for b in CASES[name][3] if b not in reached]
        print(f"{name}: {len(be.lines)} lines, peak {be.peak} B, {time.time() - t0:.1f} s; reached {reached}"
              + (f"; NOT reached {missing}" if missing else ""))
        if args.dump:
            os.makedirs(args.dump, exist_ok=True)
            stem = os.path.join(args.dump, name.replace(":", "_"))
            with open(stem + ".txt", "w") as f:
                f.write("\n".join(be.lines) + "\n")
            if args.values:
                with open(stem + ".results.txt", "w") as f:
                    for k in sorted(results):
                        v = results[k]
                        f.write(f"{k} {'None' if v is None else hashlib.sha256(v.tobytes()).hexdigest()}\n")
    if not args.cases:
        never = sorted(set(BRANCHES) - reached_all)
        print("branches never reached:", never or "none")
    path = args.out or (None if (args.values or args.cases) else os.path.join(ROOT, "tests", "golden", "engine_op_trace.json"))
    if path:
        with open(path, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
            f.write("\n")
        print("wrote", path)


if __name__ == "__main__":
    main()
