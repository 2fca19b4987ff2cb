"""Phonon q-meshes on the device (uf3_phonon_mesh / _dos / _thermo) against the host route they replace.

    python tools/bench_phonon.py [--out profiles/phonon_bench.json] [--repeats 5] [--host-q 512]

Workloads: bcc W (tests/golden/model_unary.json) -- the primitive cell (N = 1) on 64^3 and 96^3 meshes, the conventional cell
(N = 2) on 48^3, a 16-atom 2 x 2 x 2 supercell on 16^3 --, meshes reduced by time reversal.  Per workload: ms of the mesh
eigenvalues, of the smeared DOS on 2000 sample points and of 100 temperatures, each the median wall time of whole host-entry
calls (copies in and out included, the call ends in a stream synchronise) after one warm-up; q-points / s; and the host route
of the parent commit, ``frequencies_from(dynamical_matrices(...))``, timed on the first ``--host-q`` points of the same mesh and
scaled per q-point.  With UF3_PHONON_WAVE=1 in the environment the N <= 2 cells run the wave-per-q kernel instead of the
lane-per-q one (the comparison DESIGN.md section 3.12 reports).  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from uf3_amd.data.atoms import Atoms  # noqa: E402
from uf3_amd.forcefield import calculator, harmonic  # noqa: E402
from uf3_amd.regression import least_squares as ls  # noqa: E402

A0 = 3.17352
MASS = 183.84


def cells():
    prim = Atoms(numbers=[74], positions=[[0, 0, 0]], cell=0.5 * A0 * np.array([[-1, 1, 1], [1, -1, 1], [1, 1, -1]]), pbc=True)
    conv = Atoms(numbers=[74, 74], positions=[[0, 0, 0], [A0 / 2] * 3], cell=np.eye(3) * A0, pbc=True)
    base = np.array([[0, 0, 0], [0.5, 0.5, 0.5]])
    grid = np.array(list(np.ndindex(2, 2, 2)), dtype=float)
    pos = ((grid[:, None, :] + base[None]) * A0).reshape(-1, 3)
    sc16 = Atoms(numbers=[74] * 16, positions=pos, cell=np.eye(3) * 2 * A0, pbc=True)
    return [("prim_N1_mesh64", prim, (64,) * 3, 5), ("prim_N1_mesh96", prim, (96,) * 3, 5), ("conv_N2_mesh48", conv, (48,) * 3, 5),
            ("sc16_N16_mesh16", sc16, (16,) * 3, 3)]


def timed(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-q", type=int, default=512)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    model = ls.WeightedLinearModel.from_json(os.path.join(ROOT, "tests", "golden", "model_unary.json"))
    calc = calculator.UFCalculator(model, md_skin=0.0)
    res = {"model": "tests/golden/model_unary.json (W)", "a0": A0, "repeats": args.repeats,
           "forced_wave_kernel": bool(os.environ.get("UF3_PHONON_WAVE")), "workloads": {}}
    temps = np.linspace(0.0, 2000.0, 100)
    for label, atoms, mesh, n_super in cells():
        if args.only and args.only not in label:
            continue
        n = len(atoms.get_atomic_numbers())
        m = np.full(n, MASS)
        fc = harmonic._supercell_rows(calc, atoms, n_super)
        q, w = harmonic.qmesh(mesh)
        out = {"atoms": n, "mesh": list(mesh), "n_super": n_super, "q_points": len(q)}
        box = {}

        def eig():
            box["lam"], box["sweeps"] = harmonic.mesh_eigenvalues(fc, atoms, q, n_super, m, device=calc.device)

        t0 = time.perf_counter()
        terms, _ = harmonic.image_terms(atoms, n_super)
        out["image_terms_s"] = time.perf_counter() - t0
        out["n_terms"] = len(terms)
        t = timed(eig, args.repeats)
        out["mesh_eigenvalues_ms"] = 1e3 * t
        out["q_points_per_s"] = len(q) / t
        out["max_sweeps"] = int(box["sweeps"].max())
        lam = box["lam"]
        f = harmonic.eigenvalues_to_frequencies(lam)
        samples = np.linspace(f.min() - 1.0, f.max() + 1.0, 2000)
        t = timed(lambda: harmonic.dos_from_eigenvalues(lam, w, samples=samples, sigma=0.1, device=calc.device), args.repeats)
        out["smeared_dos_2000_ms"] = 1e3 * t
        out["smeared_dos_gaussians_per_s"] = lam.size * 2000 / t
        t = timed(lambda: harmonic.thermo_from_eigenvalues(lam, temps, w, device=calc.device), args.repeats)
        out["thermo_100T_ms"] = 1e3 * t
        nh = min(args.host_q, len(q))
        t0 = time.perf_counter()
        f_host = harmonic.frequencies_from(harmonic.dynamical_matrices(fc, atoms, q[:nh], n_super, m))
        th = time.perf_counter() - t0
        out["host_route_q_points"] = nh
        out["host_route_s"] = th
        out["host_route_scaled_to_mesh_s"] = th / nh * len(q)
        out["speedup_over_host_route"] = (th / nh) / (out["mesh_eigenvalues_ms"] * 1e-3 / len(q))
        lam_host = (f_host / harmonic.THZ) ** 2 * np.sign(f_host)
        out["max_rel_dev_lambda_vs_host"] = float((np.abs(lam[:nh] - lam_host).max(axis=1) / np.abs(lam_host).max(axis=1)).max())
        res["workloads"][label] = out
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
