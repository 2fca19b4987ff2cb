#!/usr/bin/env python3
"""Heat-current samples (``uf3_md_run_flux``) against the plain device MD of the same object.

    python tools/bench_flux.py [--steps 200] [--warmup 20] [--every 10] [--only NAME]

Three workloads on tests/golden/model_unary.json (bcc W, a = 3.165 A): 64 replicas of 128 atoms, one 4 000-atom frame (the
Green-Kubo size) and one 50 000-atom frame.  Per workload, on one ``MolecularDynamics`` object, each loop warmed up and ended
by a device synchronisation:
  (a) run        ``run(steps)``: the yardstick
  (b) run_flux   ``run(steps, flux_every=every)``
  (c) sample     ``UFCalculator.heat_flux`` of the final state, host arrays in and out (lists sized on every call)
Prints ms/step of (a) and (b), their ratio, ms per sample = ((b) - (a)) * every, and ms per stand-alone call of (c); writes
the JSON line to profiles/flux_bench.json as well."""
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
SKIN = 0.5


def measure(calc, frames, steps, warmup, every):
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=300.0, friction_per_fs=0.0, seed=5,
                              skin=SKIN) as dyn:
        dyn.initialize_velocities(300.0)
        dyn.run(warmup)
        dyn.run(2 * every, flux_every=every)          # (sizes the samples' lists)
        dyn.ctx.synchronize()
        t0 = time.perf_counter()
        dyn.run(steps)                                # (returns after its device synchronisation)
        plain = (time.perf_counter() - t0) / steps
        t0 = time.perf_counter()
        dyn.run(steps, flux_every=every)
        flux = (time.perf_counter() - t0) / steps
        atoms, vel = dyn.get_atoms(), dyn.get_velocities()
        masses = np.full(len(vel), MASSES["W"])
        calc.heat_flux(atoms, vel, masses)
        dyn.ctx.synchronize()
        reps = 3
        t0 = time.perf_counter()
        for _ in range(reps):
            calc.heat_flux(atoms, vel, masses)
        alone = (time.perf_counter() - t0) / reps
    return plain, flux, alone


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--only", default=None, help="one workload by name")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flux_bench.json"))
    args = ap.parse_args(argv)
    calc = calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(ROOT, "tests", "golden", "model_unary.json")),
                                   md_skin=0.0)
    workloads = {"replicas_64x128": lambda: [synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, [74], seed=300 + k) for k in range(64)],
                 "w4k": lambda: [synthetic.lattice_frame("bcc", (10, 10, 20), 3.165, [74], seed=400)],
                 "w50k": lambda: [synthetic.lattice_frame("bcc", (25, 25, 40), 3.165, [74], seed=4000)]}
    result = {}
    for name, make in workloads.items():
        if args.only and name != args.only:
            continue
        frames = make()
        n = sum(len(a) for a in frames)
        plain, flux, alone = measure(calc, frames, args.steps, args.warmup, args.every)
        row = dict(atoms=n, run_ms_per_step=round(plain * 1e3, 4), run_flux_ms_per_step=round(flux * 1e3, 4),
                   flux_over_run=round(flux / plain, 4), ms_per_sample=round((flux - plain) * args.every * 1e3, 4),
                   standalone_ms_per_call=round(alone * 1e3, 4))
        print(f"{name:16s} run {plain * 1e3:8.3f} ms/step  run+flux/{args.every} {flux * 1e3:8.3f} ms/step  ratio {flux / plain:6.3f}  "
              f"sample {row['ms_per_sample']:8.3f} ms  stand-alone {alone * 1e3:8.3f} ms")
        result[name] = row
    line = json.dumps(dict(tool="bench_flux", steps=args.steps, warmup=args.warmup, every=args.every, **result))
    print(line)
    if args.out and not args.only:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
