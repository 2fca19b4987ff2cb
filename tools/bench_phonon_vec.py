"""Eigenvectors on the q-mesh (uf3_phonon_mesh_vec / _pdos / _tdisp) against the eigenvalue-only entries and the host route.

    python tools/bench_phonon_vec.py [--out profiles/phonon_vec_bench.json] [--repeats 5] [--host-q 512] [--only LABEL]

Workloads: those of tools/bench_phonon.py (bcc W: the primitive cell on 64^3 and 96^3, the conventional cell on 48^3, a 16-atom
supercell on 16^3; meshes reduced by time reversal).  Per workload, median wall time of whole host-entry calls (copies in and out
included) after one warm-up: ``mesh_eigenvectors`` (vectors; vectors and velocities; velocities alone) against ``mesh_eigenvalues``
on the same input, the projected DOS against the total smeared DOS on 2000 sample points, the displacement tensors for 100
temperatures, and the host route (``np.linalg.eigh`` of ``dynamical_matrices``) on the first ``--host-q`` points scaled per q.
With UF3_PHONON_WAVE=1 in the environment the small cells run the wave-per-q instances.  Prints one JSON object."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from uf3_amd.forcefield import calculator, harmonic  # noqa: E402
from uf3_amd.regression import least_squares as ls  # noqa: E402
from bench_phonon import MASS, cells, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--host-q", type=int, default=512)
    ap.add_argument("--only", default=None)
    args = ap.parse_args()
    model = ls.WeightedLinearModel.from_json(os.path.join(ROOT, "tests", "golden", "model_unary.json"))
    calc = calculator.UFCalculator(model, md_skin=0.0)
    res = {"model": "tests/golden/model_unary.json (W)", "repeats": args.repeats,
           "forced_wave_kernel": bool(os.environ.get("UF3_PHONON_WAVE")), "workloads": {}}
    temps = np.linspace(0.0, 2000.0, 100)
    for label, atoms, mesh, n_super in cells():
        if args.only and args.only not in label:
            continue
        n = len(atoms.get_atomic_numbers())
        m = np.full(n, MASS)
        fc = harmonic._supercell_rows(calc, atoms, n_super)
        q, w = harmonic.qmesh(mesh)
        out = {"atoms": n, "mesh": list(mesh), "n_super": n_super, "q_points": len(q), "vector_slab": harmonic.vector_slab(3 * n)}
        box = {}

        def vectors():
            box["lam"], box["vec"] = harmonic.mesh_eigenvectors(fc, atoms, q, n_super, m, device=calc.device)

        out["mesh_eigenvalues_ms"] = 1e3 * timed(lambda: harmonic.mesh_eigenvalues(fc, atoms, q, n_super, m, device=calc.device),
                                                 args.repeats)
        out["mesh_eigenvectors_ms"] = 1e3 * timed(vectors, args.repeats)
        out["mesh_eigenvectors_and_velocities_ms"] = 1e3 * timed(
            lambda: harmonic.mesh_eigenvectors(fc, atoms, q, n_super, m, velocities=True, device=calc.device), args.repeats)
        out["mesh_velocities_only_ms"] = 1e3 * timed(
            lambda: harmonic.mesh_eigenvectors(fc, atoms, q, n_super, m, velocities=True, vectors=False, device=calc.device),
            args.repeats)
        out["eigenvector_bytes"] = int(box["vec"].nbytes)
        lam, vec = box["lam"], box["vec"]
        f = harmonic.eigenvalues_to_frequencies(lam)
        samples = np.linspace(f.min() - 1.0, f.max() + 1.0, 2000)
        out["smeared_dos_2000_ms"] = 1e3 * timed(
            lambda: harmonic.dos_from_eigenvalues(lam, w, samples=samples, sigma=0.1, device=calc.device), args.repeats)
        out["projected_dos_2000_ms"] = 1e3 * timed(
            lambda: harmonic.pdos_from_eigenvectors(lam, vec, w, samples=samples, sigma=0.1, device=calc.device), args.repeats)
        out["thermal_displacements_100T_ms"] = 1e3 * timed(
            lambda: harmonic.tdisp_from_eigenvectors(lam, vec, m, temps, w, device=calc.device), args.repeats)
        nh = min(args.host_q, len(q))
        t0 = time.perf_counter()
        D = harmonic.dynamical_matrices(fc, atoms, q[:nh], n_super, m)
        hl, hv = np.linalg.eigh(D)
        th = time.perf_counter() - t0
        out["host_route_q_points"] = nh
        out["host_route_s"] = th
        out["host_route_scaled_to_mesh_s"] = th / nh * len(q)
        out["speedup_over_host_route"] = (th / nh) / (out["mesh_eigenvectors_ms"] * 1e-3 / len(q))
        r = D @ vec[:nh] - vec[:nh] * lam[:nh, None, :]
        out["max_residual_over_norm"] = float((np.sqrt((np.abs(r) ** 2).sum(axis=1)).max(axis=1) /
                                               np.sqrt((np.abs(D) ** 2).sum(axis=(1, 2)))).max())
        res["workloads"][label] = out
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
