#!/usr/bin/env python3
"""Batched device nudged elastic bands (``uf3_amd.forcefield.neb``) against relaxation steps of the same frames.

    python tools/bench_neb.py [--steps 200] [--warmup 20] [--out profiles/neb_bench.json] [--no-full]

Two workloads (tests/golden/model_unary.json, a = 3.17352 A; first-neighbour vacancy hops in bcc W, 7 images a band):
  (a) hop64     64 bands x 7 images x 127 atoms (4 x 4 x 4 cells minus one), end points rattled differently per band: ms per NEB
                step of a fixed-length run (fmax 1e-9: nothing converges), with and without a climbing image, against ms per
                ``Relaxation`` step on the same 448 frames in the same process; and a full ``neb_bands`` run to fmax 1e-3
                between end points relaxed first (wall time, steps, barriers)
  (b) hop2k     one band of 7 x 1999 atoms (10 x 10 x 10 cells minus one): ms per step of both
Each timed loop is warmed up and ends in a device synchronisation.  Prints one JSON line last (and writes it to --out)."""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime)

from uf3_amd import synthetic  # noqa: E402
from uf3_amd.data.atoms import Atoms  # noqa: E402
from uf3_amd.forcefield import calculator, neb  # noqa: E402
from uf3_amd.forcefield.relax import Relaxation  # noqa: E402
from uf3_amd.regression import least_squares as ls  # noqa: E402

A0 = 3.17352
SKIN = 0.5


def hop_ends(reps, seed, rattle):
    """The ends of a first-neighbour vacancy hop (the atom at a (1/2, 1/2, 1/2) moves into the vacancy at 0), rattled."""
    a = synthetic.lattice_frame("bcc", reps, A0, [74], seed=0, rattle=0.0, strain=0.0)
    rng = np.random.default_rng(seed)
    x = a.get_positions()[1:]
    y = x.copy()
    y[0] = 0.0
    z = a.get_atomic_numbers()[1:]
    return (Atoms(numbers=z, positions=x + rng.normal(0, rattle, x.shape), cell=a.get_cell(), pbc=True),
            Atoms(numbers=z, positions=y + rng.normal(0, rattle, y.shape), cell=a.get_cell(), pbc=True))


def neb_step_ms(calc, bands, steps, warmup, climb):
    with neb.NudgedElasticBand(calc, bands, skin=SKIN) as band:
        band.run(warmup, fmax=1e-9, climb=climb, check_every=warmup + 1)
        t0 = time.perf_counter()
        band.run(steps, fmax=1e-9, climb=climb, check_every=steps + 1)      # (returns after its device synchronisation)
        return (time.perf_counter() - t0) / steps * 1e3


def relax_step_ms(calc, frames, steps, warmup):
    with Relaxation(calc, frames, skin=SKIN) as rel:
        rel.run(warmup, fmax=1e-9, check_every=warmup + 1)
        t0 = time.perf_counter()
        rel.run(steps, fmax=1e-9, check_every=steps + 1)
        return (time.perf_counter() - t0) / steps * 1e3


def per_step(calc, bands, steps, warmup):
    frames = [a for b in bands for a in b]
    row = dict(bands=len(bands), images=len(bands[0]), atoms=sum(len(a) for a in frames))
    row["neb_ms_per_step"] = round(neb_step_ms(calc, bands, steps, warmup, False), 4)
    row["neb_climb_ms_per_step"] = round(neb_step_ms(calc, bands, steps, warmup, True), 4)
    row["relax_ms_per_step"] = round(relax_step_ms(calc, frames, steps, warmup), 4)
    row["neb_over_relax"] = round(row["neb_ms_per_step"] / row["relax_ms_per_step"], 4)
    row["neb_climb_over_relax"] = round(row["neb_climb_ms_per_step"] / row["relax_ms_per_step"], 4)
    return row


def full_run(calc, n_bands, fmax=1e-3, max_steps=3000):
    ends = [a for k in range(n_bands) for a in hop_ends((4, 4, 4), 100 + k, 0.05)]
    t0 = time.perf_counter()
    ends, info = calc.relax_frames(ends, fmax=0.1 * fmax, max_steps=max_steps, skin=SKIN)
    relax_wall = time.perf_counter() - t0
    bands = [neb.interpolate(ends[2 * k], ends[2 * k + 1], 7) for k in range(n_bands)]
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _, out = calc.neb_bands(bands, fmax=fmax, climb=True, max_steps=max_steps, skin=SKIN)
    wall = time.perf_counter() - t0
    b = out["barrier"]
    return dict(wall_s=round(wall, 4), end_point_relaxation_wall_s=round(relax_wall, 4), bands=n_bands,
                end_points_converged=int(np.sum(info["converged"])), converged=int(np.sum(out["converged"])),
                max_steps=int(out["steps"].max()), mean_steps=round(float(out["steps"].mean()), 1),
                barrier_eV=dict(mean=round(float(b.mean()), 6), min=round(float(b.min()), 6), max=round(float(b.max()), 6)),
                reverse_barrier_eV_mean=round(float(out["reverse_barrier"].mean()), 6),
                climbing_images=sorted(set(int(c) for c in out["climbing_image"])))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-full", action="store_true", help="per-step figures only (a short run under a profiler)")
    args = ap.parse_args(argv)
    torch.cuda.init()
    model = ls.WeightedLinearModel.from_json(os.path.join(ROOT, "tests", "golden", "model_unary.json"))
    calc = calculator.UFCalculator(model, md_skin=0.0)
    result = {}

    bands = [neb.interpolate(*hop_ends((4, 4, 4), 100 + k, 0.05), 7) for k in range(64)]
    row = per_step(calc, bands, args.steps, args.warmup)
    if not args.no_full:
        row["full"] = full_run(calc, 64)
    result["hop64"] = row
    print("hop64", json.dumps(row))

    big = [neb.interpolate(*hop_ends((10, 10, 10), 7, 0.02), 7)]
    row = per_step(calc, big, args.steps, args.warmup)
    result["hop2k"] = row
    print("hop2k", json.dumps(row))
    line = json.dumps(dict(tool="bench_neb", steps=args.steps, warmup=args.warmup, **result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
