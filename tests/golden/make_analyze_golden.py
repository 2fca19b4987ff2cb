#!/usr/bin/env python3
"""
Golden capture of the reference's pair-distance histograms: uf3.data.analyze.DataAnalyzer (raw accumulators and the
analyze() dict) and uf3.representation.distances.summarize_distances.  Runs only in the build container, like
make_surface_golden.py (same stand-ins, reference at /root/reference):

    python tests/golden/make_analyze_golden.py

The stand-in ase.Atoms has no rattle(); the one ASE ships (RandomState(seed=42).normal added to the positions) is attached to
it here.  For every case frame and every setting below, tests/golden/analyze_<case>.npz holds

    <s>_keys, <s>_hist, <s>_pairs_acc      raw histogram_values / pairs_acc after load_entries([frame]), keys ascending
    <s>_totals, <s>_sizes, <s>_volumes, <s>_compositions
    <s>_a_*                                the analyze() dict per pair of the chemical system (or <s>_a_error)
    sd_hist, sd_edges, sd_lower            summarize_distances(r_cut=SD_R_CUT, n_bins=SD_N_BINS)
"""
import contextlib
import io
import json
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.join(HERE, "_standins"))
sys.path.insert(0, REF)
warnings.simplefilter("ignore")

import ase  # noqa: E402  (stand-in)
from uf3.data import composition as rc  # noqa: E402
from uf3.data import analyze as ra  # noqa: E402
from uf3.representation import distances as rd  # noqa: E402


def _rattle(self, stdev=0.001, seed=None, rng=None):
    if rng is None:
        rng = np.random.RandomState(42 if seed is None else seed)
    self.set_positions(self.positions + rng.normal(scale=stdev, size=self.positions.shape))


ase.Atoms.rattle = _rattle

CASES = ["case_steel", "case_w16", "case_nexe32", "case_ternary24_slab", "case_h2o", "case_ch4"]
# name -> DataAnalyzer settings
SETTINGS = {"plain": dict(r_cut=10.0, bins=0.05, rattle=0.0),
            "intbins": dict(r_cut=8.0, bins=150, rattle=0.0),
            "rattle": dict(r_cut=10.0, bins=0.02, rattle=0.05)}
SD_R_CUT, SD_N_BINS = 10.0, 100


def frame(d):
    return ase.Atoms(numbers=d["numbers"], positions=d["positions"], cell=d["cell"], pbc=d["pbc"])


def capture(case):
    d = np.load(os.path.join(HERE, case + ".npz"))
    meta = json.loads(str(d["meta"]))
    cs = rc.ChemicalSystem(meta["element_list"], 2)
    out = {"settings": np.array(json.dumps(SETTINGS)), "pairs": np.array([list(p) for p in cs.interactions_map[2]])}
    for name, kw in SETTINGS.items():
        an = ra.DataAnalyzer(cs, progress=None, **kw)
        an.load_entries([frame(d)])
        keys = sorted(an.histogram_values)
        out[f"{name}_keys"] = np.array(keys, dtype=np.int64)
        out[f"{name}_hist"] = np.array([an.histogram_values[k] for k in keys])
        out[f"{name}_pairs_acc"] = np.array([an.pairs_acc[k] for k in keys], dtype=np.int64)
        out[f"{name}_totals"] = np.array(an.totals_acc, dtype=np.int64)
        out[f"{name}_sizes"] = np.array(an.sizes)
        out[f"{name}_volumes"] = np.array(an.volumes)
        out[f"{name}_compositions"] = np.array(an.compositions)
        try:
            with contextlib.redirect_stdout(io.StringIO()):
                res = an.analyze()
        except KeyError as e:
            out[f"{name}_a_error"] = np.array(repr(e))
            continue
        out[f"{name}_a_bin_edges"] = res["bin_edges"]
        out[f"{name}_a_atomic_volumes"] = np.array([res["atomic_volumes"][el] for el in cs.element_list])
        for p, pair in enumerate(cs.interactions_map[2]):
            out[f"{name}_a_hist{p}"] = res["histograms"][pair]
            if pair not in res["rdfs"]:
                continue
            out[f"{name}_a_rdf{p}"] = res["rdfs"][pair]
            out[f"{name}_a_reference{p}"] = res["reference"][pair]
            out[f"{name}_a_coverage{p}"] = np.array(res["coverage"][pair])
            out[f"{name}_a_lower{p}"] = np.array(res["lower_bounds"][pair])
            out[f"{name}_a_peaks{p}"] = res["peaks"][pair]
            out[f"{name}_a_valleys{p}"] = res["valleys"][pair]
    with contextlib.redirect_stdout(io.StringIO()):
        try:
            hist, edges, lower = rd.summarize_distances([frame(d)], cs, r_cut=SD_R_CUT, n_bins=SD_N_BINS,
                                                        print_stats=True, progress=None)
            out["sd_hist"] = np.array([hist[p] for p in cs.interactions_map[2]])
            out["sd_edges"] = edges
            out["sd_lower"] = np.array([lower[p] for p in cs.interactions_map[2]])
        except IndexError as e:                 # a pair never observed: the reference's lower-bound lookup fails
            out["sd_error"] = np.array(repr(e))
    np.savez_compressed(os.path.join(HERE, f"analyze_{case}.npz"), **out)
    print(case, sorted(k for k in out if k.endswith("error")))


if __name__ == "__main__":
    for c in CASES:
        capture(c)
