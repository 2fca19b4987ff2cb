#!/usr/bin/env python3
"""
Pair-distance histogram throughput (uf3_pair_histogram_dev; DataAnalyzer.load_entries): N config_c4 frames (10 000-atom W/Mo
bcc cells) at r_cut = 12 A, 0.01 A bins (1200 bins x 3 pairs), upper bound inclusive, no rattle.

    python tools/bench_analyze.py [--frames 64] [--reps 5] [--out profiles/analyze_bench.json]

Reports device-event time of one uf3_pair_histogram_dev call on the whole batch (frames/s, kept pairs/s; candidates/s from
the cell list's candidate count of frame 0 times the frames, all frames share the lattice), host-inclusive
DataAnalyzer.load_entries frames/s, and -- labelled CPU -- the NumPy restatement of the reference's counting (chunked scipy
cdist against the explicit supercell + np.histogram) on ONE frame.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpu", action="store_true", help="also time the CPU restatement on one frame")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from uf3_amd import _lib, synthetic
    from uf3_amd.data import analyze, composition

    frames = [synthetic.config_c4(f)[0] for f in range(args.frames)]
    r_cut, species = 12.0, [42, 74]
    an0 = analyze.DataAnalyzer(composition.ChemicalSystem(["Mo", "W"], 2), r_cut=r_cut, bins=0.01, progress=None)
    edges = an0.bin_edges
    db = analyze._hist_basis(species, 0.0, r_cut)
    fb = _lib.FrameBatch(frames)
    pos = torch.from_numpy(fb.pos).cuda()
    z = torch.from_numpy(fb.z).cuda()
    out = torch.zeros((3, len(edges) - 1), dtype=torch.int64, device="cuda")
    stream = torch.cuda.current_stream()
    prev = db.ctx.set_stream(stream.cuda_stream)
    times = []
    try:
        for rep in range(args.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            _lib.pair_histogram_dev(db, fb.struct, pos.data_ptr(), z.data_ptr(), out.data_ptr(), edges)
            e1.record(stream)
            torch.cuda.synchronize()
            if rep:
                times.append(e0.elapsed_time(e1) / 1e3)
    finally:
        db.ctx.restore_stream(prev)
    kept = int(out.sum().item())
    t_dev = float(np.median(times))
    # candidates per atom: the cell list's scan (bins of >= r_cut / 2 per axis, two bins to either side: 5 x 5 x 5 bins) at the
    # frame's density -- an estimate, the kernel does not count them
    cell = np.asarray(frames[0].get_cell())
    vol = abs(np.linalg.det(cell))
    heights = [vol / np.linalg.norm(np.cross(cell[(k + 1) % 3], cell[(k + 2) % 3])) for k in range(3)]
    scan = np.prod([5 * h / np.floor(h / (0.5 * r_cut)) for h in heights])
    cand_per_atom = len(frames[0]) / vol * scan
    n_atoms = fb.n_atoms
    # host-inclusive analyzer (frames already built)
    an = analyze.DataAnalyzer(composition.ChemicalSystem(["Mo", "W"], 2), r_cut=r_cut, bins=0.01, progress=None)
    an.load_entries(frames[:2])
    an.clear()
    t0 = time.perf_counter()
    an.load_entries(frames)
    t_host = time.perf_counter() - t0
    assert an.totals_acc == kept, (an.totals_acc, kept)
    res = dict(workload=f"{args.frames} x config_c4 (10000 atoms, W/Mo), r_cut 12 A, 0.01 A bins, inclusive",
               device_s=t_dev, device_frames_per_s=args.frames / t_dev, kept_pairs=kept, kept_pairs_per_s=kept / t_dev,
               est_candidates_per_s=cand_per_atom * n_atoms / t_dev,
               load_entries_s=t_host, load_entries_frames_per_s=args.frames / t_host, reps=args.reps)
    if args.cpu:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        from test_gpu_analyze import restated
        t0 = time.perf_counter()
        ref = restated(frames[0], species, edges, r_cut, True)
        res["cpu_restatement_one_frame_s"] = time.perf_counter() - t0
        res["cpu_restatement_frames_per_s"] = 1.0 / res["cpu_restatement_one_frame_s"]
        one, _ = analyze.pair_histograms([frames[0]], species, edges, 0.0, r_cut)
        res["cpu_restatement_equal"] = bool(np.array_equal(one, ref))
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
