#!/usr/bin/env python3
"""Per-atom extrapolation grades on the device (``uf3_site_grade_dev``) against the routes that existed before it, and the cost
of sampling them inside a molecular-dynamics run.

    python tools/bench_site_grade.py [--reps 5] [--rounds 5] [--only NAME] [--md-steps 100] [--out FILE]

Two batches of the bench's W/Mo 2+3-body basis (F = 434): 64 frames of 128 atoms and one frame of 10 000 atoms.  The whitening
matrix is that of the batch's own force Gram plus the default regulariser (tools/bench_leverage.py's).  Per batch, positions
resident in HBM:
  (a) site_grade      ``uf3_site_grade_dev``: lists, rows in LDS, W on the matrix cores, the frames' maxima
  (b) rows_leverage   ``uf3_site_rows_dev`` into HBM + ``uf3_leverage_dev(group=1)``: the un-fused pair
  (c) force_rows      ``DeviceLeverage.frames(forces=True)`` from host frames: the per-atom route there was before (3N force
                      rows through HBM); host clock, uploads included -- (d) is its like-for-like partner
  (d) sites           ``DeviceLeverage.sites`` from host frames, host clock
(a) and (b) are timed with device events around ``reps`` calls, alternating over ``rounds`` rounds; the median per call is
reported with the spread (min .. max) of the rounds.
MD: ``run(n)`` against ``run(n, grade_every=10)`` on 64 x 128 atoms (Mo/W) and on one 50 000-atom W frame (``--md-large 0``
skips it: a sample's list build is O(N^2 images) per frame), host clock around the whole run, alternating, after a warm-up run.
Prints one JSON line; writes it to profiles/site_grade_bench.json unless ``--only`` or ``--out ''``."""
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

from uf3_amd import _lib, pipeline, synthetic  # noqa: E402
from uf3_amd.forcefield import calculator  # noqa: E402
from uf3_amd.forcefield.md import MolecularDynamics  # noqa: E402
from uf3_amd.regression import least_squares as ls  # noqa: E402
from uf3_amd.representation import process  # noqa: E402

NUMS = [42, 74]
MASSES = {"Mo": 95.95, "W": 183.84}


def batch_model(basis, fz, frames):
    """A model whose system matrix is the batch's own force Gram (unit mean diagonal) + the default regulariser."""
    x_f = fz.featurize_frames(frames[:4], energy=False)[1]
    x_f = x_f.reshape(-1, x_f.shape[-1])[:30000]
    model = ls.WeightedLinearModel(basis)
    mask = np.asarray(model.mask)
    gram = (x_f.T @ x_f)[np.ix_(mask, mask)]
    reg = ls.freeze_regularizer(model.regularizer, mask)
    model.system_matrix = gram / np.mean(np.diag(gram)) + reg.T @ reg
    model.coefficients = np.random.default_rng(1).normal(0, 0.01, model.n_feats)
    model.coefficients[np.asarray(model.col_idx, dtype=int)] = 0.0
    return model


def measure(basis, fz, frames, reps, rounds):
    ctx, db = fz._dev()
    dev = torch.device("cuda", ctx.device)
    batch = _lib.FrameBatch(frames)
    F, n = db.n_feat, batch.n_atoms
    model = batch_model(basis, fz, frames)
    w = torch.from_numpy(model.whitening()).to(dev)
    d_pos, d_z = torch.from_numpy(batch.pos).to(dev), torch.from_numpy(batch.z).to(dev)
    g = torch.empty(n, dtype=torch.float64, device=dev)
    g2 = torch.empty(n, dtype=torch.float64, device=dev)
    fm = torch.empty(batch.n_frames, dtype=torch.float64, device=dev)
    fa = torch.empty(batch.n_frames, dtype=torch.int32, device=dev)
    rows = torch.empty((n, F), dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    prev = ctx.set_stream(stream.cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    try:
        def site_grade():
            ctx.check(ctx.lib.uf3_site_grade_dev(db.handle, C.byref(batch.struct), p(d_pos), p(d_z), p(w), p(g), p(fm), p(fa)))

        def rows_leverage():
            ctx.check(ctx.lib.uf3_site_rows_dev(db.handle, C.byref(batch.struct), p(d_pos), p(d_z), p(rows), F))
            ctx.check(ctx.lib.uf3_leverage_dev(ctx.handle, p(rows), n, F, F, p(w), 1, p(g2)))

        calls = {"site_grade": site_grade, "rows_leverage": rows_leverage}
        for call in calls.values():
            for _ in range(2):
                call()
                ctx.synchronize()
        a, b = g.cpu().numpy(), g2.cpu().numpy()
        agree = float(np.abs(a - b).max() / np.abs(b).max())
        times = {k: [] for k in calls}
        for _ in range(rounds):
            for name, call in calls.items():
                ctx.synchronize()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                for _ in range(reps):
                    call()
                t1.record(stream)
                t1.synchronize()
                ctx.synchronize()
                times[name].append(t0.elapsed_time(t1) * 1e-3 / reps)
    finally:
        ctx.restore_stream(prev)
    lev = pipeline.DeviceLeverage(model, fz)
    host = {"force_rows": lambda: lev.frames(frames, forces=True), "sites": lambda: lev.sites(frames)}
    for call in host.values():
        call()
    for name in host:
        times[name] = []
    for _ in range(rounds):
        for name, call in host.items():
            t0 = time.perf_counter()
            call()
            times[name].append(time.perf_counter() - t0)
    row = dict(frames=batch.n_frames, atoms=n, n_feat=F, max_rel_diff_fused_to_unfused=agree)
    for name, t in times.items():
        row[name + "_ms"] = round(float(np.median(t)) * 1e3, 4)
        row[name + "_ms_min_max"] = [round(min(t) * 1e3, 4), round(max(t) * 1e3, 4)]
    row["site_grade_over_rows_leverage"] = round(row["site_grade_ms"] / row["rows_leverage_ms"], 3)
    row["sites_over_force_rows"] = round(row["sites_ms"] / row["force_rows_ms"], 3)
    return row


def measure_md(basis, fz, frames, n_steps, rounds, every=10):
    model = batch_model(basis, fz, frames)
    calc = calculator.UFCalculator(model)
    dyn = MolecularDynamics(calc, frames, 1.0, masses=MASSES, temperature_K=300.0, friction_per_fs=0.01, seed=1)
    dyn.initialize_velocities(300.0, seed=2)
    dyn.run(every, grade_every=every)                      # warm-up: lists sized, W uploaded, kernels loaded
    dyn.run(every)
    times = {"plain": [], "graded": []}
    for _ in range(rounds):
        for name, kw in (("plain", {}), ("graded", dict(grade_every=every))):
            t0 = time.perf_counter()
            dyn.run(n_steps, **kw)
            times[name].append(time.perf_counter() - t0)
    row = dict(frames=len(frames), atoms=int(sum(len(a) for a in frames)), steps=n_steps, grade_every=every)
    for name, t in times.items():
        row[name + "_ms_per_step"] = round(float(np.median(t)) * 1e3 / n_steps, 4)
        row[name + "_ms_per_step_min_max"] = [round(min(t) * 1e3 / n_steps, 4), round(max(t) * 1e3 / n_steps, 4)]
    row["graded_over_plain"] = round(row["graded_ms_per_step"] / row["plain_ms_per_step"], 3)
    row["ms_per_sample"] = round((row["graded_ms_per_step"] - row["plain_ms_per_step"]) * every, 4)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", default=None, help="one workload by name")
    ap.add_argument("--md-steps", type=int, default=100)
    ap.add_argument("--md-large", type=int, default=1, help="0: skip the 50 000-atom MD workload")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "site_grade_bench.json"))
    args = ap.parse_args(argv)
    basis = synthetic.notebook_basis(['Mo', 'W'])
    fz = process.BasisFeaturizer(basis)
    small = lambda: [synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, NUMS, seed=500 + k) for k in range(64)]     # noqa: E731
    workloads = {"frames_64x128": lambda: measure(basis, fz, small(), args.reps, args.rounds),
                 "frames_1x10000": lambda: measure(basis, fz, [synthetic.config_c4(frame=0)[0]], args.reps, args.rounds),
                 "md_64x128": lambda: measure_md(basis, fz, small(), args.md_steps, args.rounds)}
    if args.md_large:
        workloads["md_1x50000"] = lambda: measure_md(
            basis, fz, [synthetic.lattice_frame("bcc", (30, 30, 28), 3.165, [74], seed=900)], max(args.md_steps // 5, 20), 3)
    result = {}
    for name, run in workloads.items():
        if args.only and name != args.only:
            continue
        row = run()
        print(f"{name:16s} " + "  ".join(f"{k} {row[k]}" for k in row if k.endswith("_ms") or k.endswith("_per_step") or "over" in k),
              flush=True)
        result[name] = row
    line = json.dumps(dict(tool="bench_site_grade", build_id=_lib.build_id(), reps=args.reps, rounds=args.rounds, **result))
    print(line)
    if args.out and not args.only:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
