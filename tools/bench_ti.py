#!/usr/bin/env python3
"""What a switching step (``MolecularDynamics.switch``, uf3_amd/csrc/uf3_ti.h) costs over a ``run`` step of the same object.

    python tools/bench_ti.py [--steps 200] [--warmup 20] [--repeats 3] [--out profiles/ti_bench.json]

tools/bench_md.py's two workloads (tests/golden/model_unary.json, bcc W, a = 3.165 A, 300 K): 64 replicas of 128 atoms, and one
50 000-atom frame.  Langevin (friction 0.01 / fs).  Per workload one object; ``run`` and ``switch`` (lambda 0.2 -> 0.9, springs
of 5 eV / A^2 on the sites the object started from) with the centre of mass held and not, alternating ``--repeats`` times, each
call of ``--steps`` steps, each starting with one list build and ending in its own device synchronisation.  The figure of a loop
is the median over the repeats.  Prints one JSON line last (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (before the library: one HIP runtime)

from uf3_amd import synthetic  # noqa: E402
from uf3_amd.forcefield import calculator, md  # noqa: E402
from uf3_amd.regression import least_squares as ls  # noqa: E402

MASSES = {"W": 183.84}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    calc = calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(ROOT, "tests", "golden", "model_unary.json")),
                                   md_skin=0.0)
    workloads = {"replicas_64x128": [synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, [74], seed=300 + k) for k in range(64)],
                 "w50k": [synthetic.lattice_frame("bcc", (25, 25, 40), 3.165, [74], seed=4000)]}
    result = {}
    for name, frames in workloads.items():
        n = sum(len(a) for a in frames)
        with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=300.0, friction_per_fs=0.01, seed=5) as dyn:
            dyn.initialize_velocities(300.0)
            dyn.set_reference(None, 5.0)
            loops = {"run": lambda k: dyn.run(k),
                     "switch": lambda k: dyn.switch(k, 0.2, 0.9, fix_com=False),
                     "switch_fix_com": lambda k: dyn.switch(k, 0.2, 0.9, fix_com=True)}
            for fn in loops.values():
                fn(args.warmup)
            times = {key: [] for key in loops}
            for _ in range(args.repeats):
                for key, fn in loops.items():
                    dyn.ctx.synchronize()
                    t0 = time.perf_counter()
                    fn(args.steps)
                    times[key].append((time.perf_counter() - t0) / args.steps)
        row = {key: dict(ms_per_step=round(float(np.median(t)) * 1e3, 4), all_ms_per_step=[round(x * 1e3, 4) for x in t])
               for key, t in times.items()}
        for key in ("switch", "switch_fix_com"):
            row[key + "_over_run"] = round(row[key]["ms_per_step"] / row["run"]["ms_per_step"], 4)
        row["atoms"] = n
        print(f"{name:16s} run {row['run']['ms_per_step']:.4f} ms/step  switch {row['switch']['ms_per_step']:.4f} "
              f"({row['switch_over_run']:.3f}x)  switch, fixed centre of mass {row['switch_fix_com']['ms_per_step']:.4f} "
              f"({row['switch_fix_com_over_run']:.3f}x)")
        result[name] = row
    line = json.dumps(dict(tool="bench_ti", steps=args.steps, warmup=args.warmup, repeats=args.repeats, **result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
