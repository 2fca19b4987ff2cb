#!/usr/bin/env python3
"""Batched device relaxation (``uf3_amd.forcefield.relax``) against NVE MD steps of the same batch and ``relax_fmax``.

    python tools/bench_relax.py [--steps 200] [--warmup 20]

Three workloads (tests/golden/model_unary.json, a = 3.17352 A):
  (a) vac64     64 rattled 127-atom W vacancy cells, positions only: a full relaxation to fmax 1e-3 (wall time, steps, and
                the share of evaluator work spent on frames that had already converged), plus ms per step of a fixed-length
                run (fmax 1e-9: nothing converges) against ``MolecularDynamics.run`` (NVE) on the same batch
  (b) vac54k    one 53 999-atom W frame with a vacancy: ms per step of relaxation and of NVE MD
  (c) cell64    64 strained 128-atom cells with the cell as a degree of freedom: ms per step, and a full relaxation to 1e-3
Each timed loop is warmed up and ends in a device synchronisation.  ``relax_fmax`` (host FIRE, one frame at a time) is timed
on a few frames of each workload (for (b) over --fmax-steps steps) and scaled to the batch for the speed-up.  Prints one JSON
line last."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime)

from uf3_amd import synthetic  # noqa: E402
from uf3_amd.data.atoms import Atoms  # noqa: E402
from uf3_amd.forcefield import calculator, md  # noqa: E402
from uf3_amd.forcefield.relax import Relaxation  # noqa: E402
from uf3_amd.regression import least_squares as ls  # noqa: E402

A0 = 3.17352
SKIN = 0.5


def vacancy(reps, seed, rattle=0.05):
    a = synthetic.lattice_frame("bcc", reps, A0, [74], seed=seed, rattle=rattle, strain=0.0)
    return Atoms(numbers=a.get_atomic_numbers()[1:], positions=a.get_positions()[1:], cell=a.get_cell(), pbc=True)


def strained(seed):
    rng = np.random.default_rng(seed)
    a = synthetic.lattice_frame("bcc", (4, 4, 4), A0, [74], seed=seed, rattle=0.02, strain=0.0)
    eps = rng.uniform(-0.02, 0.02, (3, 3))
    eps = 0.5 * (eps + eps.T)
    return Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions() @ (np.eye(3) + eps),
                 cell=np.asarray(a.get_cell()) @ (np.eye(3) + eps), pbc=True)


def relax_step_ms(calc, frames, steps, warmup, relax_cell):
    with Relaxation(calc, frames, relax_cell=relax_cell, skin=SKIN) as rel:
        rel.run(warmup, fmax=1e-9, check_every=warmup + 1)
        t0 = time.perf_counter()
        rel.run(steps, fmax=1e-9, check_every=steps + 1)       # (returns after its device synchronisation)
        return (time.perf_counter() - t0) / steps * 1e3


def md_step_ms(calc, frames, steps, warmup):
    with md.MolecularDynamics(calc, frames, 1.0, masses={"W": 183.84}, skin=SKIN) as dyn:
        dyn.initialize_velocities(300.0, seed=3)
        dyn.run(warmup)
        dyn.ctx.synchronize()
        t0 = time.perf_counter()
        dyn.run(steps)
        return (time.perf_counter() - t0) / steps * 1e3


def full_relax(calc, frames, relax_cell, fmax=1e-3, max_steps=2000):
    with Relaxation(calc, frames[:2], relax_cell=relax_cell, skin=SKIN) as rel:      # (warm-up: kernels, lists, basis)
        rel.run(20, fmax=fmax)
    with Relaxation(calc, frames, relax_cell=relax_cell, skin=SKIN) as rel:
        t0 = time.perf_counter()
        out = rel.run(max_steps, fmax=fmax)
        wall = time.perf_counter() - t0
    steps = out["steps"]
    return dict(wall_s=round(wall, 4), converged=int(np.sum(out["converged"])), frames=len(frames), max_steps=int(steps.max()),
                mean_steps=round(float(steps.mean()), 1),
                useful_eval_share=round(float((steps + 1).sum()) / (len(frames) * float(steps.max() + 1)), 4))


def host_relax(calc, frames, relax_cell, fmax=1e-3, max_steps=2000):
    calc.relax_fmax(frames[0], fmax=fmax, relax_cell=relax_cell, max_steps=5, timeout=1e9)    # (warm-up)
    t0 = time.perf_counter()
    for a in frames:
        calc.relax_fmax(a, fmax=fmax, relax_cell=relax_cell, max_steps=max_steps, timeout=1e9)
    return (time.perf_counter() - t0) / len(frames)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--host-frames", type=int, default=3)
    ap.add_argument("--fmax-steps", type=int, default=20)
    args = ap.parse_args(argv)
    torch.cuda.init()
    model = ls.WeightedLinearModel.from_json(os.path.join(ROOT, "tests", "golden", "model_unary.json"))
    calc = calculator.UFCalculator(model, md_skin=0.0)
    host_calc = calculator.UFCalculator(model)                   # (relax_fmax with the calculator's default "auto" skin)
    result = {}

    vac = [vacancy((4, 4, 4), 100 + k) for k in range(64)]
    row = dict(atoms=sum(len(a) for a in vac))
    row["relax_ms_per_step"] = round(relax_step_ms(calc, vac, args.steps, args.warmup, False), 4)
    row["md_ms_per_step"] = round(md_step_ms(calc, vac, args.steps, args.warmup), 4)
    row["relax_over_md"] = round(row["relax_ms_per_step"] / row["md_ms_per_step"], 4)
    row["full"] = full_relax(calc, vac, False)
    per_frame = host_relax(host_calc, vac[:args.host_frames], False)
    row["relax_fmax_s_per_frame"] = round(per_frame, 4)
    row["speedup_vs_relax_fmax"] = round(per_frame * len(vac) / row["full"]["wall_s"], 2)
    result["vac64"] = row
    print("vac64", json.dumps(row))

    big = [vacancy((30, 30, 30), 7, rattle=0.02)]
    row = dict(atoms=len(big[0]))
    row["relax_ms_per_step"] = round(relax_step_ms(calc, big, args.steps, args.warmup, False), 4)
    row["md_ms_per_step"] = round(md_step_ms(calc, big, args.steps, args.warmup), 4)
    row["relax_over_md"] = round(row["relax_ms_per_step"] / row["md_ms_per_step"], 4)
    host_calc.relax_fmax(big[0], fmax=1e-9, relax_cell=False, max_steps=3, timeout=1e9)
    t0 = time.perf_counter()
    host_calc.relax_fmax(big[0], fmax=1e-9, relax_cell=False, max_steps=args.fmax_steps, timeout=1e9)
    row["relax_fmax_ms_per_step"] = round((time.perf_counter() - t0) / args.fmax_steps * 1e3, 4)
    row["speedup_vs_relax_fmax_per_step"] = round(row["relax_fmax_ms_per_step"] / row["relax_ms_per_step"], 2)
    result["vac54k"] = row
    print("vac54k", json.dumps(row))

    cells = [strained(500 + k) for k in range(64)]
    row = dict(atoms=sum(len(a) for a in cells))
    row["relax_ms_per_step"] = round(relax_step_ms(calc, cells, args.steps, args.warmup, True), 4)
    row["full"] = full_relax(calc, cells, True)
    per_frame = host_relax(host_calc, cells[:args.host_frames], True)
    row["relax_fmax_s_per_frame"] = round(per_frame, 4)
    row["speedup_vs_relax_fmax"] = round(per_frame * len(cells) / row["full"]["wall_s"], 2)
    result["cell64"] = row
    print("cell64", json.dumps(row))
    print(json.dumps(dict(tool="bench_relax", steps=args.steps, warmup=args.warmup, **result)))


if __name__ == "__main__":
    main()
