#!/usr/bin/env python
"""Record tests/golden/forward_launches.json: for every row of tests/forward_plan_cases.py, what one forward on a live engine
launched - the launch count per profile label (Engine.profile, Engine.profile_entries), Engine.last_plan and Engine.last_split of
the seven conv layers.  Needs an MI355X.  It asks the engine nothing a build before csrc/plan.h's decide_forward lacks, so the file
can be (and was) recorded with the library as it stood before the forward's launches were decided apart from their issuing.

    python tools/record_forward_launches.py [--out tests/golden/forward_launches.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import forward_plan_cases as FP                                       # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "forward_launches.json"))
    args = ap.parse_args()
    rows = []
    for r in FP.ROWS:
        rows.append(dict(id=FP.row_id(r), **FP.observe(r)))
        print(rows[-1]["id"], rows[-1]["launches"], flush=True)
    with open(args.out, "w") as f:
        f.write("{\"rows\": [\n" + ",\n".join(json.dumps(row, sort_keys=True, separators=(",", ":")) for row in rows) + "\n]}\n")
    print("wrote %d rows to %s" % (len(rows), args.out))


if __name__ == "__main__":
    main()
