#!/usr/bin/env python3
"""Leverage on the device (``uf3_leverage_dev``) against the torch route on the same buffers and against featurizing the batch.

    python tools/bench_leverage.py [--reps 10] [--rounds 7] [--only NAME] [--out FILE]

Two batches of the bench's W/Mo 2+3-body basis (F = 434), resident in HBM: one frame of 10 000 atoms (30 000 force rows) and 64
frames of 128 atoms (24 576 force rows).  The whitening matrix W is that of the batch's own weighted Gram plus the default
regulariser.  Per batch, on the force rows already in HBM:
  (a) leverage        ``uf3_leverage_dev(x_f, W, group=3)``: no scratch, the triangle of W only
  (b) torch           ``((X @ W.T) ** 2).view(-1, 3, F).sum((1, 2))``: dense GEMM through the vendor library, Z = X W^T in HBM
  (c) featurize       ``uf3_featurize_dev(x_e, x_f)`` of the batch, the cost of making the rows
and end to end from host frames
  (d) frames          ``DeviceLeverage.frames`` (upload, featurize, leverage, read q back)
Every call is warmed up; (a)-(c) are timed with device events around ``reps`` calls on the stream all three run on, alternating
over ``rounds`` rounds, (d) with a host clock; the median per call is reported with the spread (min .. max) of the rounds.
Prints one JSON line; writes it to profiles/leverage_bench.json unless ``--only`` or ``--out ''``."""
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
from uf3_amd.regression import least_squares as ls  # noqa: E402
from uf3_amd.representation import process  # noqa: E402

NUMS = [42, 74]


def measure(basis, fz, frames, reps, rounds):
    ctx, db = fz._dev()
    dev = torch.device("cuda", ctx.device)
    batch = _lib.FrameBatch(frames)
    F = db.n_feat
    d_pos, d_z = torch.from_numpy(batch.pos).to(dev), torch.from_numpy(batch.z).to(dev)
    x_e = torch.empty((batch.n_frames, F), dtype=torch.float64, device=dev)
    x_f = torch.empty((batch.n_atoms * 3, F), dtype=torch.float64, device=dev)
    q = torch.empty(batch.n_atoms, dtype=torch.float64, device=dev)
    stream = torch.cuda.current_stream(dev)
    prev = ctx.set_stream(stream.cuda_stream)
    try:
        fz.featurize_device(batch.struct, d_pos.data_ptr(), d_z.data_ptr(), x_e.data_ptr(), x_f.data_ptr())
        ctx.synchronize()
        # a model whose system matrix is this batch's own: force Gram (scaled to unit mean diagonal) + the default regulariser
        model = ls.WeightedLinearModel(basis)
        mask = np.asarray(model.mask)
        gram = (x_f.T @ x_f).cpu().numpy()[np.ix_(mask, mask)]
        reg = ls.freeze_regularizer(model.regularizer, mask)
        model.system_matrix = gram / np.mean(np.diag(gram)) + reg.T @ reg
        model.coefficients = np.zeros(F)
        w_host = model.whitening()
        w = torch.from_numpy(w_host).to(dev)

        def leverage():
            ctx.check(ctx.lib.uf3_leverage_dev(ctx.handle, C.c_void_p(x_f.data_ptr()), x_f.shape[0], F, F, C.c_void_p(w.data_ptr()), 3,
                                               C.c_void_p(q.data_ptr())))

        q_torch = [None]

        def torch_route():
            q_torch[0] = ((x_f @ w.T) ** 2).view(-1, 3, F).sum((1, 2))

        def featurize():
            fz.featurize_device(batch.struct, d_pos.data_ptr(), d_z.data_ptr(), x_e.data_ptr(), x_f.data_ptr())

        calls = {"leverage": leverage, "torch": torch_route, "featurize": featurize}
        for call in calls.values():
            for _ in range(3):
                call()
                ctx.synchronize()
        # both routes give the same numbers (the torch route is the comparator of the timing, not of the tests)
        ref = q_torch[0].cpu().numpy()
        agree = float(np.abs(q.cpu().numpy() - ref).max() / np.abs(ref).max())
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
    for _ in range(2):
        lev.frames(frames)
    times["frames"] = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        lev.frames(frames)
        times["frames"].append(time.perf_counter() - t0)
    row = dict(frames=batch.n_frames, atoms=batch.n_atoms, rows=int(x_f.shape[0]), n_feat=F, max_rel_diff_to_torch=agree)
    for name, t in times.items():
        row[name + "_ms"] = round(float(np.median(t)) * 1e3, 4)
        row[name + "_ms_min_max"] = [round(min(t) * 1e3, 4), round(max(t) * 1e3, 4)]
    row["leverage_over_torch"] = round(row["leverage_ms"] / row["torch_ms"], 3)
    row["leverage_over_featurize"] = round(row["leverage_ms"] / row["featurize_ms"], 3)
    row["leverage_gflops_triangle"] = round(x_f.shape[0] * F * (F + 1) / (row["leverage_ms"] * 1e-3) / 1e9, 1)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default=None, help="one batch by name")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "leverage_bench.json"))
    args = ap.parse_args(argv)
    basis = synthetic.notebook_basis(['Mo', 'W'])
    fz = process.BasisFeaturizer(basis)
    workloads = {"frames_1x10000": lambda: [synthetic.config_c4(frame=0)[0]],
                 "frames_64x128": lambda: [synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, NUMS, seed=500 + k) for k in range(64)]}
    result = {}
    for name, make in workloads.items():
        if args.only and name != args.only:
            continue
        row = measure(basis, fz, make(), args.reps, args.rounds)
        print(f"{name:16s} " + "  ".join(f"{k[:-3]} {row[k]:9.3f} ms" for k in row if k.endswith("_ms")))
        result[name] = row
    line = json.dumps(dict(tool="bench_leverage", build_id=_lib.build_id(), reps=args.reps, rounds=args.rounds, **result))
    print(line)
    if args.out and not args.only:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
