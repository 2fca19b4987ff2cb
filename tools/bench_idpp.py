#!/usr/bin/env python3
"""IDPP band initialisation on the device (``neb.IDPP``, ``neb.idpp_interpolate``) beside NEB steps of the same frames.

    python tools/bench_idpp.py [--steps 200] [--warmup 20] [--out profiles/idpp_bench.json]

Two workloads (first-neighbour vacancy hops in bcc W, a = 3.17352 A, 7 images a band; tools/bench_neb.py's frames):
  (a) hop64     64 bands x 7 images x 127 atoms: ms per IDPP step of a fixed-length run (fmax 1e-12: nothing converges) against
                ms per ``NudgedElasticBand`` step (tests/golden/model_unary.json) of the same frames in the same process; and
                the wall time of ``idpp_interpolate`` to fmax 0.1 (ASE's default) and to 1e-3 for the 64 bands (steps, bands
                converged)
  (b) hop2k     one band of 7 x 1999 atoms: ms per step of both
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402  (before the library: one HIP runtime)

from uf3_amd.forcefield import calculator, neb  # noqa: E402
from uf3_amd.regression import least_squares as ls  # noqa: E402
from bench_neb import hop_ends, neb_step_ms  # noqa: E402


def idpp_step_ms(bands, steps, warmup):
    with neb.IDPP(bands) as band:
        band.run(warmup, fmax=1e-12, check_every=warmup + 1)
        t0 = time.perf_counter()
        band.run(steps, fmax=1e-12, check_every=steps + 1)                  # (returns after its device synchronisation)
        return (time.perf_counter() - t0) / steps * 1e3


def per_step(calc, bands, steps, warmup):
    row = dict(bands=len(bands), images=len(bands[0]), atoms=sum(len(a) for b in bands for a in b))
    row["idpp_ms_per_step"] = round(idpp_step_ms(bands, steps, warmup), 4)
    row["neb_ms_per_step"] = round(neb_step_ms(calc, bands, steps, warmup, False), 4)
    row["idpp_over_neb"] = round(row["idpp_ms_per_step"] / row["neb_ms_per_step"], 4)
    return row


def full_run(ends, fmax=0.1):
    t0 = time.perf_counter()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        _, out = neb.idpp_interpolate([e[0] for e in ends], [e[1] for e in ends], 7, fmax=fmax)
    wall = time.perf_counter() - t0
    return dict(wall_s=round(wall, 4), bands=len(ends), fmax=fmax, converged=int(np.sum(out["converged"])),
                max_steps=int(out["steps"].max()), mean_steps=round(float(out["steps"].mean()), 1))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    torch.cuda.init()
    model = ls.WeightedLinearModel.from_json(os.path.join(ROOT, "tests", "golden", "model_unary.json"))
    calc = calculator.UFCalculator(model, md_skin=0.0)
    result = {}

    ends = [hop_ends((4, 4, 4), 100 + k, 0.05) for k in range(64)]
    row = per_step(calc, [neb.interpolate(a, b, 7) for a, b in ends], args.steps, args.warmup)
    full_run(ends[:2])                                                      # (warm: the first call's one-off costs)
    row["full"] = full_run(ends)
    row["full_fmax_1e-3"] = full_run(ends, fmax=1e-3)                       # (a straight hop's linear band already meets 0.1)
    result["hop64"] = row
    print("hop64", json.dumps(row))

    big = [neb.interpolate(*hop_ends((10, 10, 10), 7, 0.02), 7)]
    row = per_step(calc, big, args.steps, args.warmup)
    result["hop2k"] = row
    print("hop2k", json.dumps(row))
    line = json.dumps(dict(tool="bench_idpp", steps=args.steps, warmup=args.warmup, **result))
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
