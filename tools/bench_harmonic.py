"""Device Hessian (uf3_hessian) against the finite-displacement route it replaces, and the phonon / elastic drivers on bcc W.

    python tools/bench_harmonic.py [--out profiles/harmonic_bench.json] [--skip-fd]

Cases: a 2000-atom bcc W frame (10 x 10 x 10 conventional cells) -- H alone and H with the strain terms --, a 1000-row slab
of a 54 000-atom frame, the same 2000-atom H by central differences of UFCalculator.evaluate_frames (6N displaced frames in
batches), and end-to-end get_phonon_data / get_elastic_constants.  Wall times of whole calls (host copies included), median
of the repeats after one warm-up.  Prints one JSON object."""
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


def bcc(reps, a=A0, rattle=0.0, seed=0):
    base = np.array([[0, 0, 0], [0.5, 0.5, 0.5]])
    grid = np.array(list(np.ndindex(*reps)), dtype=float)
    pos = ((grid[:, None, :] + base[None]) * a).reshape(-1, 3)
    pos += np.random.default_rng(seed).normal(0, rattle, pos.shape)
    return Atoms(numbers=np.full(len(pos), 74), positions=pos, cell=np.diag(np.array(reps, dtype=float) * a), pbc=True)


class _W(Atoms):
    def get_masses(self):
        return np.full(len(self.get_atomic_numbers()), 183.84)


def timed(fn, repeats):
    fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--skip-fd", action="store_true")
    args = ap.parse_args()
    model = ls.WeightedLinearModel.from_json(os.path.join(ROOT, "tests", "golden", "model_unary.json"))
    calc = calculator.UFCalculator(model, md_skin=0.0)
    res = {"model": "tests/golden/model_unary.json (W)", "a0": A0}
    w2k = bcc((10, 10, 10), rattle=0.02, seed=1)
    n = len(w2k.get_atomic_numbers())
    t, ts = timed(lambda: harmonic.hessian(calc, w2k), args.repeats)
    res["hessian_2000_s"] = t
    res["hessian_2000_bytes_out"] = 9 * n * n * 8
    t, _ = timed(lambda: harmonic.hessian(calc, w2k, strain=True), args.repeats)
    res["hessian_strain_2000_s"] = t
    big = bcc((30, 30, 30), rattle=0.02, seed=2)
    res["slab_atoms"] = len(big.get_atomic_numbers())
    t, _ = timed(lambda: harmonic.hessian(calc, big, rows=(0, 1000)), args.repeats)
    res["hessian_slab_1000_of_54000_s"] = t
    if not args.skip_fd:
        H = harmonic.hessian(calc, w2k)
        pos = np.asarray(w2k.get_positions(), dtype=float)
        h = 1e-5
        batch = 200
        Hfd = np.empty_like(H)
        t0 = time.perf_counter()
        for k0 in range(0, 3 * n, batch // 2):
            ks = range(k0, min(k0 + batch // 2, 3 * n))
            frames = []
            for k in ks:
                for sgn in (1, -1):
                    p = pos.copy()
                    p[k // 3, k % 3] += sgn * h
                    frames.append(Atoms(numbers=w2k.get_atomic_numbers(), positions=p, cell=w2k.get_cell(), pbc=True))
            f = calc.evaluate_frames(frames)[1].reshape(len(ks), 2, 3 * n)
            Hfd[:, k0:k0 + len(ks)] = -(f[:, 0] - f[:, 1]).T / (2 * h)
        res["finite_difference_2000_s"] = time.perf_counter() - t0
        res["finite_difference_frames"] = 6 * n
        res["finite_difference_max_rel_dev"] = float(np.abs(Hfd - H).max() / np.abs(H).max())
    conv = _W(numbers=[74, 74], positions=[[0, 0, 0], [A0 / 2] * 3], cell=np.eye(3) * A0, pbc=True)
    t, _ = timed(lambda: calc.get_phonon_data(conv, n_super=5), args.repeats)
    res["get_phonon_data_conventional_n5_s"] = t
    t, _ = timed(lambda: calc.get_elastic_constants(conv), args.repeats)
    res["get_elastic_constants_s"] = t
    res["elastic_C11_C12_C44_B_GPa"] = calc.get_elastic_constants(conv)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
