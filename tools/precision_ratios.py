#!/usr/bin/env python
"""
Collect the ``[precision] route, case: kind ratio, ...`` lines of a ``pytest -s tests/test_gpu_precision.py
tests/test_gpu_precision_d2.py tests/test_gpu_precision_mc.py`` run into ``profiles/precision_ratios.json``: route by case by kind, the worst ratio where a line
repeats, beside the bound the run was held to.  A ratio is ``max |device - extended oracle| / (2^-53 M)`` over every entry of a
result (tests/_precision.py).  Several logs may be given (one per test file, say): their routes are merged.

    python -m pytest -m gpu -s tests/test_gpu_precision.py tests/test_gpu_precision_d2.py tests/test_gpu_precision_mc.py | tee precision.log
    python tools/precision_ratios.py precision.log [-o profiles/precision_ratios.json]

``--update`` keeps the routes already in the output file that the logs do not mention (a run of one of the three test files).
"""
import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LINE = re.compile(r"\[precision\] (?P<route>.+), (?P<case>\w+): (?P<kinds>(?:\w+ [-+.\deE]+(?:, )?)+)\s*$")


def collect(lines):
    out = {}
    for line in lines:
        m = LINE.search(line)
        if not m or m.group("route").startswith(("fp64 oracle", "planted")):
            continue
        slot = out.setdefault(m.group("route"), {}).setdefault(m.group("case"), {})
        for item in m.group("kinds").split(", "):
            kind, value = item.split()
            slot[kind] = max(slot.get(kind, 0.0), float(value))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("log", nargs="+")
    ap.add_argument("-o", "--out", default=os.path.join(ROOT, "profiles", "precision_ratios.json"))
    ap.add_argument("--update", action="store_true", help="keep the output file's routes that the logs do not mention")
    args = ap.parse_args()
    lines = []
    for path in args.log:
        with open(path, errors="replace") as f:
            lines += f.read().splitlines()
    routes = collect(lines)
    if not routes:
        sys.exit("no [precision] lines found")
    if args.update and os.path.exists(args.out):
        with open(args.out) as f:
            routes = {**json.load(f)["routes"], **routes}
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import _precision as P
    worst = {}
    for cases in routes.values():
        for kinds in cases.values():
            for k, v in kinds.items():
                worst[k] = max(worst.get(k, 0.0), v)
    doc = {"what": "worst |device - extended oracle| / (2^-53 M) over every entry, per route, case and kind of output "
                   "(xe, xf, xv: energy, force, virial rows; e, f, v: energy, forces, virial: tests/test_gpu_precision.py; "
                   "H, mixed, born: Hessian, position / strain and strain / strain derivatives; U, W, jp: site energies, site "
                   "virials, the heat current's potential part; b: site rows: tests/test_gpu_precision_d2.py; dE: Monte Carlo energy "
                   "differences, and the running energy of a chain in units of its own bound's sum: tests/test_gpu_precision_mc.py)",
           "rho_o": P.RHO_O, "gamma": P.GAMMA, "worst": worst, "routes": routes}
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(routes)} routes, worst {worst} -> {args.out}")


if __name__ == "__main__":
    main()
