#!/usr/bin/env python3
"""Device MD (``uf3_amd.forcefield.md``) against the evaluator's MD-route walk of ``bench.py`` (extra ``eval_50k``).

    python tools/bench_md.py [--steps 200] [--warmup 20]

One process, two workloads: one 50 000-atom bcc-W frame (tests/golden/model_unary.json, a = 3.165 A) and 64 replicas of
128 atoms.  Three loops of the same length per workload, each warmed up and ended by a device synchronisation:
  (a) walk      a seeded +-0.01 A random walk applied with torch ``add_`` + ``uf3_eval_dev`` (skin 0.5 A)
  (b) nve       ``MolecularDynamics.run`` at friction 0 (velocity Verlet), 300 K initial velocities
  (c) langevin  the same with friction 0.01 / fs at 300 K (BAOAB)
  (d) nve_stress  (b) recording the stress on every step: the strain derivative every step, as constant pressure needs it
  (e) nph       constant pressure 0, barostat time 500 fs, no friction (uf3_md_run_npt)
  (f) npt       the same with friction 0.01 / fs on the atoms and 0.002 / fs on the piston
Prints ms/step, atom-steps/s, the ratios (b)/(a) and (c)/(a) and the neighbour-list builds of each loop, then one JSON line.
(b) and (c) time one ``run`` call each, which starts with one list build."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime)

from uf3_amd import _lib, synthetic  # noqa: E402
from uf3_amd.forcefield import calculator, md  # noqa: E402
from uf3_amd.regression import least_squares as ls  # noqa: E402

MASSES = {"W": 183.84}
SKIN = 0.5
WALK = 0.01


def walk_loop(calc, frames, steps, warmup, dev):
    ctx = _lib.get_context(dev.index)
    db = _lib.device_basis(calc.bspline_config, ctx)
    batch = _lib.FrameBatch(frames)
    n = batch.n_atoms
    d_pos = torch.from_numpy(batch.pos).to(dev)
    d_z = torch.from_numpy(batch.z).to(dev)
    d_e = torch.empty((batch.n_frames,), dtype=torch.float64, device=dev)
    d_f = torch.empty((n, 3), dtype=torch.float64, device=dev)
    g = torch.Generator(device=dev).manual_seed(17)
    pool = (torch.rand((16, n, 3), dtype=torch.float64, device=dev, generator=g) * 2.0 - 1.0) * WALK
    fields = [pool[i] for i in range(16)]
    picks = [int(x) for x in np.random.default_rng(17).integers(0, 16, steps + warmup)]
    alphas = [float(x) for x in np.random.default_rng(18).choice([-1.0, 1.0], steps + warmup)]
    prev = ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    skin0 = getattr(ctx, "_md_skin", 0.0)
    ctx.md_skin(SKIN)
    args = (db.handle, C.byref(batch.struct), C.c_void_p(d_pos.data_ptr()), C.c_void_p(d_z.data_ptr()), _lib._p(calc._c1),
            _lib._p(calc._c2), _lib._p(calc._c3), C.c_void_p(d_e.data_ptr()), C.c_void_p(d_f.data_ptr()))
    try:
        def step(k):
            d_pos.add_(fields[picks[k]], alpha=alphas[k])
            rc = ctx.lib.uf3_eval_dev(*args)
            if rc:
                ctx.check(rc)
        for k in range(warmup):
            step(k)
        torch.cuda.synchronize(dev)
        b0 = ctx.md_stats()["builds"]
        t0 = time.perf_counter()
        for k in range(steps):
            step(warmup + k)
        torch.cuda.synchronize(dev)
        dt = (time.perf_counter() - t0) / steps
        return dt, ctx.md_stats()["builds"] - b0
    finally:
        ctx.md_skin(skin0)
        ctx.restore_stream(prev)


def md_loop(calc, frames, steps, warmup, friction, stress=False, **barostat):
    with md.MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=300.0, friction_per_fs=friction, seed=5,
                              skin=SKIN, **barostat) as dyn:
        dyn.initialize_velocities(300.0)
        dyn.run(warmup)
        ctx = dyn.ctx
        ctx.synchronize()
        b0 = ctx.md_stats()["builds"]
        t0 = time.perf_counter()
        if stress:
            dyn.run(steps, thermo_every=1, stress=True)
        else:
            dyn.run(steps)                   # (returns after its device synchronisation)
        dt = (time.perf_counter() - t0) / steps
        return dt, ctx.md_stats()["builds"] - b0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args(argv)
    dev = torch.device("cuda", 0)
    calc = calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(ROOT, "tests", "golden", "model_unary.json")),
                                   md_skin=0.0)
    workloads = {"w50k": [synthetic.lattice_frame("bcc", (25, 25, 40), 3.165, [74], seed=4000)],
                 "replicas_64x128": [synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, [74], seed=300 + k) for k in range(64)]}
    result = {}
    for name, frames in workloads.items():
        n = sum(len(a) for a in frames)
        row = {}
        for loop, fn in (("walk", lambda: walk_loop(calc, frames, args.steps, args.warmup, dev)),
                         ("nve", lambda: md_loop(calc, frames, args.steps, args.warmup, 0.0)),
                         ("langevin", lambda: md_loop(calc, frames, args.steps, args.warmup, 0.01)),
                         ("nve_stress", lambda: md_loop(calc, frames, args.steps, args.warmup, 0.0, stress=True)),
                         ("nph", lambda: md_loop(calc, frames, args.steps, args.warmup, 0.0, pressure_eV_A3=0.0,
                                                 barostat_time_fs=500.0)),
                         ("npt", lambda: md_loop(calc, frames, args.steps, args.warmup, 0.01, pressure_eV_A3=0.0,
                                                 barostat_time_fs=500.0, barostat_friction_per_fs=0.002))):
            dt, builds = fn()
            row[loop] = dict(ms_per_step=round(dt * 1e3, 4), atom_steps_per_s=round(n / dt), builds=int(builds))
            print(f"{name:16s} {loop:10s} {dt * 1e3:8.3f} ms/step  {n / dt / 1e6:8.1f} M atom-steps/s  builds {builds}")
        row["nve_over_walk"] = round(row["nve"]["ms_per_step"] / row["walk"]["ms_per_step"], 4)
        row["langevin_over_walk"] = round(row["langevin"]["ms_per_step"] / row["walk"]["ms_per_step"], 4)
        for loop in ("nph", "npt"):
            row[loop + "_over_nve"] = round(row[loop]["ms_per_step"] / row["nve"]["ms_per_step"], 4)
            row[loop + "_over_nve_stress"] = round(row[loop]["ms_per_step"] / row["nve_stress"]["ms_per_step"], 4)
        row["atoms"] = n
        print(f"{name:16s} nve/walk {row['nve_over_walk']:.3f}  langevin/walk {row['langevin_over_walk']:.3f}  "
              f"nph/nve {row['nph_over_nve']:.3f}  npt/nve {row['npt_over_nve']:.3f}  nph/nve+stress {row['nph_over_nve_stress']:.3f}  "
              f"npt/nve+stress {row['npt_over_nve_stress']:.3f}")
        result[name] = row
    print(json.dumps(dict(tool="bench_md", steps=args.steps, warmup=args.warmup, **result)))


if __name__ == "__main__":
    main()
