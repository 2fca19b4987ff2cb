#!/usr/bin/env python3
"""Virial rows (``uf3_featurize_virial_dev``) against the featurizer's own calls on the same batch.

    python tools/bench_virial_rows.py [--reps 20] [--rounds 7] [--only NAME] [--out FILE]

Two batches of the bench's W/Mo 2+3-body basis (F = 434): 64 frames of 128 atoms and 8 frames of 10 000 atoms, resident in
HBM.  Per batch three device-entry calls, outputs in HBM:
  (a) energy_rows          ``uf3_featurize_dev(x_e, NULL)``: the yardstick for "energy rows only"
  (b) energy_virial_rows   ``uf3_featurize_virial_dev(x_e, NULL, x_v)``
  (c) energy_force_rows    ``uf3_featurize_dev(x_e, x_f)``: 3 N rows a frame where (b) writes six
Every call is warmed up (capacities learnt, code objects loaded); a measurement is a host clock around ``reps`` calls ended by a
device synchronisation, and the three calls alternate over ``rounds`` rounds: the median per call is reported with the spread
(min .. max) of the rounds.  A library without the virial entry (an earlier commit's, for the yardstick) reports (a) and (c).
Prints one JSON line; writes it to profiles/virial_rows_bench.json unless ``--only`` or ``--out ''``."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402  (before the library: one HIP runtime)

from uf3_amd import _lib, synthetic  # noqa: E402
from uf3_amd.representation import process  # noqa: E402

NUMS = [42, 74]


def measure(fz, frames, reps, rounds):
    ctx, db = fz._dev()
    dev = torch.device("cuda", ctx.device)
    batch = _lib.FrameBatch(frames)
    F = db.n_feat
    d_pos, d_z = torch.from_numpy(batch.pos).to(dev), torch.from_numpy(batch.z).to(dev)
    x_e = torch.empty((batch.n_frames, F), dtype=torch.float64, device=dev)
    x_f = torch.empty((batch.n_atoms * 3, F), dtype=torch.float64, device=dev)
    x_v = torch.empty((batch.n_frames, 6, F), dtype=torch.float64, device=dev)
    has_virial = hasattr(ctx.lib, "uf3_featurize_virial_dev")
    calls = {"energy_rows": lambda: fz.featurize_device(batch.struct, d_pos.data_ptr(), d_z.data_ptr(), x_e.data_ptr(), None),
             "energy_force_rows": lambda: fz.featurize_device(batch.struct, d_pos.data_ptr(), d_z.data_ptr(), x_e.data_ptr(),
                                                              x_f.data_ptr())}
    if has_virial:
        calls["energy_virial_rows"] = lambda: fz.featurize_device(batch.struct, d_pos.data_ptr(), d_z.data_ptr(), x_e.data_ptr(),
                                                                  None, d_x_v=x_v.data_ptr())
    prev = ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        for call in calls.values():                 # warm-up: capacities, code objects
            for _ in range(3):
                call()
                ctx.synchronize()
        times = {k: [] for k in calls}
        for _ in range(rounds):
            for name, call in calls.items():
                ctx.synchronize()
                t0 = time.perf_counter()
                for _ in range(reps):
                    call()
                ctx.synchronize()
                times[name].append((time.perf_counter() - t0) / reps)
    finally:
        ctx.restore_stream(prev)
    row = dict(frames=batch.n_frames, atoms=batch.n_atoms, n_feat=F)
    for name, t in times.items():
        row[name + "_ms"] = round(float(np.median(t)) * 1e3, 4)
        row[name + "_ms_min_max"] = [round(min(t) * 1e3, 4), round(max(t) * 1e3, 4)]
    if has_virial:
        row["virial_over_energy"] = round(row["energy_virial_rows_ms"] / row["energy_rows_ms"], 3)
        row["virial_over_force"] = round(row["energy_virial_rows_ms"] / row["energy_force_rows_ms"], 3)
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--only", default=None, help="one batch by name")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "virial_rows_bench.json"))
    args = ap.parse_args(argv)
    fz = process.BasisFeaturizer(synthetic.notebook_basis(['Mo', 'W']))
    workloads = {"frames_64x128": lambda: [synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, NUMS, seed=500 + k) for k in range(64)],
                 "frames_8x10000": lambda: [synthetic.config_c4(frame=k)[0] for k in range(8)]}
    result = {}
    for name, make in workloads.items():
        if args.only and name != args.only:
            continue
        reps = args.reps if name == "frames_64x128" else max(3, args.reps // 4)
        row = measure(fz, make(), reps, args.rounds)
        print(f"{name:16s} " + "  ".join(f"{k[:-3]} {row[k]:9.3f} ms" for k in row if k.endswith("_ms")))
        result[name] = row
    line = json.dumps(dict(tool="bench_virial_rows", build_id=_lib.build_id(), reps=args.reps, rounds=args.rounds, **result))
    print(line)
    if args.out and not args.only:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
