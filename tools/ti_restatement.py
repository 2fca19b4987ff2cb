#!/usr/bin/env python3
"""The Frenkel-Ladd protocol of tests/test_gpu_ti.py's physics test run twice: through the NumPy restatement of the switching
scheme (tests/_ti_ref.py) with the device evaluator for its forces, and through the device driver
(``free_energy.frenkel_ladd``).  Not a test: it says what the protocol itself gives on this model before the device's
integrator enters -- the mean Delta F, its standard error and its distance from the harmonic value -- so that the step counts
of the test are long enough for the restatement alone.

    python tools/ti_restatement.py [--replicas 64] [--equilibrate 1000] [--switch 3000] [--out FILE.json]

One evaluator call per step on the host route: minutes, where the device driver takes seconds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import torch  # noqa: E402,F401  (before the library: one HIP runtime)

from uf3_amd import synthetic  # noqa: E402
from uf3_amd.forcefield import free_energy as fe, md  # noqa: E402
from uf3_amd.forcefield.md import KB  # noqa: E402
from _md_ref import init_velocities  # noqa: E402
from _ti_ref import constrained_logdet, run_switch  # noqa: E402
from test_gpu_md import MASSES, _forces_of, _unary  # noqa: E402


def summary(delta, diss, harmonic):
    n = len(delta)
    return dict(delta_F=float(delta.mean()), standard_error=float(delta.std(ddof=1) / np.sqrt(n)),
                distance_from_harmonic=float(delta.mean() - harmonic), dissipation=float(diss.mean()),
                dissipation_standard_error=float(diss.std(ddof=1) / np.sqrt(n)))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--replicas", type=int, default=64)
    ap.add_argument("--equilibrate", type=int, default=1000)
    ap.add_argument("--switch", type=int, default=3000)
    ap.add_argument("--temperature", type=float, default=100.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    calc = _unary()
    atoms = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=0, rattle=0.0, strain=0.0)
    n, temp, n_rep = len(atoms), args.temperature, args.replicas
    hess = calc.get_hessian(atoms)
    hess = 0.5 * (hess + hess.T)
    spring = float(np.mean(np.diag(hess)))
    masses = md.resolve_masses([atoms], MASSES)
    eig = np.linalg.eigvalsh(hess)
    harmonic = float(calc.evaluate_frames([atoms])[0][0] + 0.5 * KB * temp * (
        constrained_logdet(hess, masses) - constrained_logdet(spring * np.eye(3 * n), masses)))
    result = dict(tool="ti_restatement", replicas=n_rep, equilibrate=args.equilibrate, switch=args.switch, temperature_K=temp,
                  atoms=n, spring=spring, hessian_eigenvalues=[float(eig[0]), float(eig[3]), float(eig[-1])], harmonic=harmonic,
                  allowance_cap=0.05 * 3 * (n - 1) * KB * temp)
    print(json.dumps(result), flush=True)

    t0 = time.perf_counter()
    out = fe.frenkel_ladd(calc, atoms, temp, masses=MASSES, n_replicas=n_rep, n_equilibrate=args.equilibrate, n_switch=args.switch,
                          spring=spring, friction_per_fs=0.02, seed=17)
    result["device"] = dict(summary(out["delta_F"][0], out["dissipation"][0], harmonic), seconds=round(time.perf_counter() - t0, 2),
                            free_energy=float(out["free_energy"][0]))
    print(json.dumps(result["device"]), flush=True)

    frames = [atoms] * n_rep
    forces_of, off = _forces_of(calc, frames)
    m = np.tile(masses, n_rep)
    sites = np.tile(atoms.get_positions(), (n_rep, 1))
    k = np.full(len(m), spring)
    x, v = sites.copy(), init_velocities(m, off, temp, 17, 0)
    sched, step, work, block = fe.switching_schedule(args.switch, "smooth"), 0, {}, 500
    t0 = time.perf_counter()
    for name, lo, hi in (("forward", 0.0, 1.0), ("backward", 1.0, 0.0)):
        for n_steps, table in ((args.equilibrate, np.zeros(args.equilibrate + 1)), (args.switch, sched)):
            lam_b = lo if table is not sched else hi
            total = np.zeros(n_rep)
            for first in range(0, n_steps, block):              # (in blocks, so that the run says where it is)
                last = min(first + block, n_steps)
                x, v, w, _ = run_switch(x, v, m, forces_of, off, sites, k, last - first, 1.0, temp, 0.02, 17, lo, lam_b,
                                        table[first:last + 1], True, step0=step)
                total, step = total + w, step + last - first
                print(f"restatement: step {step}  ({time.perf_counter() - t0:.0f} s)", flush=True)
            if table is sched:
                work[name] = total
    result["restatement"] = dict(summary(0.5 * (work["forward"] - work["backward"]), 0.5 * (work["forward"] + work["backward"]),
                                         harmonic), seconds=round(time.perf_counter() - t0, 2))
    line = json.dumps(result)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
