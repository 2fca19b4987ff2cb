#!/usr/bin/env python3
"""What periodic wrapping and MSD samples cost a device MD run (``MolecularDynamics(wrap=True)``, ``run(msd_every=10)``).

    python tools/bench_md_wrap.py [--steps 200] [--warmup 20] [--repeats 3]

Two workloads, those of tools/bench_md.py: 64 replicas of 128 bcc-W atoms and one 50 000-atom frame (tests/golden/
model_unary.json, 300 K, NVE, skin 0.5 A).  Three loops per workload, each an object of its own, warmed up, ``repeats`` timed
``run`` calls, the best kept:
  (a) plain     wrap=False, ``run(n)``
  (b) wrap      wrap=True, ``run(n)``: one ``k_md_wrap`` launch in front of every list build
  (c) wrap_msd  wrap=True, ``run(n, msd_every=10)``: two small launches per sample on top
Prints ms/step, the neighbour-list builds of the timed run (``uf3_ctx_md_stats``) and the ratios (b)/(a), (c)/(a), then one
JSON line."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before the library: one HIP runtime)

from uf3_amd import synthetic  # noqa: E402
from uf3_amd.forcefield import calculator, md  # noqa: E402
from uf3_amd.regression import least_squares as ls  # noqa: E402

MASSES = {"W": 183.84}
SKIN = 0.5
MSD_EVERY = 10


def loop(calc, frames, steps, warmup, repeats, wrap, msd_every):
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=300.0, seed=5, skin=SKIN, wrap=wrap) as dyn:
        dyn.initialize_velocities(300.0)
        dyn.run(warmup, msd_every=msd_every if warmup >= msd_every else 0)
        ctx = dyn.ctx
        best, builds = None, 0
        for _ in range(repeats):
            ctx.synchronize()
            b0 = ctx.md_stats()["builds"]
            t0 = time.perf_counter()
            dyn.run(steps, msd_every=msd_every)          # (returns after its device synchronisation)
            dt = (time.perf_counter() - t0) / steps
            if best is None or dt < best:
                best, builds = dt, ctx.md_stats()["builds"] - b0
        return best, builds


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args(argv)
    calc = calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(ROOT, "tests", "golden", "model_unary.json")),
                                   md_skin=0.0)
    workloads = {"replicas_64x128": [synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, [74], seed=300 + k) for k in range(64)],
                 "w50k": [synthetic.lattice_frame("bcc", (25, 25, 40), 3.165, [74], seed=4000)]}
    result = {}
    for name, frames in workloads.items():
        n = sum(len(a) for a in frames)
        row = {}
        for which, wrap, every in (("plain", False, 0), ("wrap", True, 0), ("wrap_msd", True, MSD_EVERY)):
            dt, builds = loop(calc, frames, args.steps, args.warmup, args.repeats, wrap, every)
            row[which] = dict(ms_per_step=round(dt * 1e3, 4), atom_steps_per_s=round(n / dt), builds=int(builds))
            print(f"{name:16s} {which:9s} {dt * 1e3:8.4f} ms/step  {n / dt / 1e6:8.1f} M atom-steps/s  builds {builds}")
        row["wrap_over_plain"] = round(row["wrap"]["ms_per_step"] / row["plain"]["ms_per_step"], 4)
        row["wrap_msd_over_plain"] = round(row["wrap_msd"]["ms_per_step"] / row["plain"]["ms_per_step"], 4)
        row["atoms"] = n
        print(f"{name:16s} wrap/plain {row['wrap_over_plain']:.3f}  wrap+msd/plain {row['wrap_msd_over_plain']:.3f}")
        result[name] = row
    print(json.dumps(dict(tool="bench_md_wrap", steps=args.steps, warmup=args.warmup, repeats=args.repeats, msd_every=MSD_EVERY,
                          **result)))


if __name__ == "__main__":
    main()
