#!/usr/bin/env python3
"""Device species-swap Monte Carlo (``uf3_amd.forcefield.mc``) against the route without it: one evaluator call per trial.

    python tools/bench_mc.py [--trials 20000] [--warmup 2000] [--eval-trials 100] [--out profiles/mc_bench.json]

Two workloads (``synthetic.notebook_basis(["Mo", "W"])``, seeded coefficients, rattled bcc cells, a = 3.165 A, 1000 K):
  (a) alloy64   64 frames x 128 atoms (4 x 4 x 4 cells): one trial of every frame per step
  (b) alloy2k   one frame of 2000 atoms (10 x 10 x 10 cells)
For each: trials per second and microseconds per trial (a "trial" is one trial of EVERY frame of the batch) of ``MonteCarlo.run``
in swap mode, and of the whole-frame route -- per trial, two atoms of every frame exchange their species on the host and
``UFCalculator.evaluate_frames`` (energies only) evaluates the batch again.  Each timed loop is warmed up and ends in a device
synchronisation.  Prints one JSON line last (and writes it to --out)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime)

from uf3_amd import _lib, synthetic  # noqa: E402
from uf3_amd.data.atoms import Atoms  # noqa: E402
from uf3_amd.forcefield import calculator, mc  # noqa: E402
from uf3_amd.regression import least_squares as ls  # noqa: E402


def make_calc():
    basis = synthetic.notebook_basis(["Mo", "W"])
    model = ls.WeightedLinearModel(basis)
    coeff = np.random.default_rng(31).normal(0, 0.05, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    model.coefficients = coeff
    return calculator.UFCalculator(model, md_skin=0.0)


def mc_us_per_trial(calc, frames, trials, warmup):
    t0 = time.perf_counter()
    chain = mc.MonteCarlo(calc, frames, 1000.0, seed=1)
    create_s = time.perf_counter() - t0
    with chain:
        chain.run(warmup)
        t0 = time.perf_counter()
        out = chain.run(trials)                        # (returns after its device synchronisation)
        dt = time.perf_counter() - t0
    return dt / trials * 1e6, float(out["accepted"].sum() / out["trials"].sum()), create_s


def eval_us_per_trial(calc, frames, trials, warmup):
    ctx = _lib.get_context(calc.device)
    rng = np.random.default_rng(2)
    numbers = [np.asarray(a.get_atomic_numbers()).copy() for a in frames]

    def trial():
        moved = []
        for a, z in zip(frames, numbers):
            i, j = rng.integers(0, len(z), 2)
            z[i], z[j] = z[j], z[i]
            moved.append(Atoms(numbers=z, positions=a.get_positions(), cell=a.get_cell(), pbc=a.get_pbc()))
        return calc.evaluate_frames(moved, forces=False)[0]
    for _ in range(warmup):
        trial()
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(trials):
        trial()
    ctx.synchronize()
    return (time.perf_counter() - t0) / trials * 1e6


def workload(calc, frames, args):
    row = dict(frames=len(frames), atoms=sum(len(a) for a in frames))
    us, acc, create_s = mc_us_per_trial(calc, frames, args.trials, args.warmup)
    row["mc_us_per_trial"] = round(us, 3)
    row["mc_trials_per_s"] = round(1e6 / us, 1)
    row["mc_frame_trials_per_s"] = round(len(frames) * 1e6 / us, 1)
    row["mc_acceptance"] = round(acc, 4)
    row["mc_create_s"] = round(create_s, 4)
    ev = eval_us_per_trial(calc, frames, args.eval_trials, max(args.eval_trials // 10, 3))
    row["eval_us_per_trial"] = round(ev, 3)
    row["eval_trials_per_s"] = round(1e6 / ev, 1)
    row["eval_over_mc"] = round(ev / us, 2)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--trials", type=int, default=20000)
    ap.add_argument("--warmup", type=int, default=2000)
    ap.add_argument("--eval-trials", type=int, default=100)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    torch.cuda.init()
    calc = make_calc()
    result = {}
    small = [synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, [42, 74], seed=500 + k, rattle=0.05) for k in range(64)]
    result["alloy64"] = workload(calc, small, args)
    print("alloy64", json.dumps(result["alloy64"]))
    big = [synthetic.lattice_frame("bcc", (10, 10, 10), 3.165, [42, 74], seed=600, rattle=0.05)]
    result["alloy2k"] = workload(calc, big, args)
    print("alloy2k", json.dumps(result["alloy2k"]))
    line = json.dumps(dict(tool="bench_mc", trials=args.trials, warmup=args.warmup, eval_trials=args.eval_trials, **result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
