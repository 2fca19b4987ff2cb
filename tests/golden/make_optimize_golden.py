#!/usr/bin/env python3
"""
Golden capture of the reference's cut-off helpers (uf3.regression.optimize): get_bspline_config, get_lower_cutoffs,
get_columns_to_drop_2b / _3b.  Runs only in the build container, like make_analyze_golden.py (same stand-ins, reference at
/root/reference):

    python tests/golden/make_optimize_golden.py

tests/golden/optimize_cases.json holds, per case (chemical system + get_bspline_config arguments):

    knots          knots_map of the basis, keys "A-B" / "A-B-C"
    lower_rmax_2b, lower_rmax_3b    get_lower_cutoffs
    drop_2b        {repr(r): get_columns_to_drop_2b(basis, r, spacing_2b)} for every lower 2-body cut-off
    drop_3b        {repr(r): get_columns_to_drop_3b(basis, r, spacing_3b)} for every lower 3-body cut-off

and "raises": the inputs of the four functions that raise ValueError, with the message.
"""
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

from uf3.data import composition as rc  # noqa: E402
from uf3.regression import optimize as ro  # noqa: E402

CONFIG_1 = dict(rmin_2b=0.01, rmax_2b=6.01, rmin_3b=0.8, rmax_3b=4, knot_spacing_2b=0.4, knot_spacing_3b=0.8)
CONFIG_2 = dict(rmin_2b=0.1, rmax_2b=9.1, rmin_3b=0.9, rmax_3b=7.2, knot_spacing_2b=0.3, knot_spacing_3b=0.9)
NOTEBOOK_W = dict(rmin_2b=0.0, rmax_2b=8.0, rmin_3b=1.6, rmax_3b=5.6, knot_spacing_2b=0.5, knot_spacing_3b=0.8)
CASES = {
    "nbsn_config_1": (["Nb", "Sn"], CONFIG_1),
    "mow_config_1": (["Mo", "W"], CONFIG_1),
    "nbsn_config_2": (["Nb", "Sn"], CONFIG_2),
    "w_notebook": (["W"], NOTEBOOK_W),
    "monbw_config_1": (["Mo", "Nb", "W"], CONFIG_1),
}
# get_bspline_config arguments that raise (on the Nb/Sn system), and drop-function cut-offs that raise (on nbsn_config_1)
RAISE_CONFIG = {
    "rmax_2b_off_grid": dict(CONFIG_1, rmax_2b=6.05),
    "rmax_3b_off_grid": dict(CONFIG_1, rmax_3b=4.1),
    "rmax_3b_double_off_grid": dict(CONFIG_1, rmin_3b=0.9, rmax_3b=4.1),
    "leading_trim": dict(CONFIG_1, leading_trim=1),
    "trailing_trim": dict(CONFIG_1, trailing_trim=2),
}
RAISE_DROP_2B = [6.2, 0.2, 7.0]
RAISE_DROP_3B = [3.0, 4.4, 0.5]


def key(interaction):
    return "-".join(interaction)


def config(elements, kw, leading_trim=0, trailing_trim=3):
    cs = rc.ChemicalSystem(list(elements), degree=3)
    return ro.get_bspline_config(cs, leading_trim=leading_trim, trailing_trim=trailing_trim, **kw)


def main():
    out = dict(cases={}, raises=dict(config={}, drop_2b={}, drop_3b={}))
    for name, (elements, kw) in CASES.items():
        basis = config(elements, kw)
        knots = {}
        for interaction, value in basis.knots_map.items():
            knots[key(interaction)] = ([np.asarray(v).tolist() for v in value] if len(interaction) == 3
                                       else np.asarray(value).tolist())
        low = ro.get_lower_cutoffs(basis)
        case = dict(elements=elements, args=kw, knots=knots, n_feat=int(np.sum(basis.get_feature_partition_sizes())),
                    lower_rmax_2b=low["lower_rmax_2b"].tolist(), lower_rmax_3b=low["lower_rmax_3b"].tolist(),
                    drop_2b={}, drop_3b={})
        for r in low["lower_rmax_2b"]:
            case["drop_2b"][repr(float(r))] = [str(c) for c in ro.get_columns_to_drop_2b(basis, r, kw["knot_spacing_2b"])]
        for r in low["lower_rmax_3b"]:
            case["drop_3b"][repr(float(r))] = [str(c) for c in ro.get_columns_to_drop_3b(basis, r, kw["knot_spacing_3b"])]
        out["cases"][name] = case
    for name, kw in RAISE_CONFIG.items():
        kw = dict(kw)
        lead, trail = kw.pop("leading_trim", 0), kw.pop("trailing_trim", 3)
        try:
            config(["Nb", "Sn"], kw, lead, trail)
        except ValueError as exc:
            out["raises"]["config"][name] = dict(args=kw, leading_trim=lead, trailing_trim=trail, message=str(exc))
        else:
            raise AssertionError(f"{name} did not raise")
    basis = config(["Nb", "Sn"], CONFIG_1)
    for which, values, fn, spacing in (("drop_2b", RAISE_DROP_2B, ro.get_columns_to_drop_2b, CONFIG_1["knot_spacing_2b"]),
                                       ("drop_3b", RAISE_DROP_3B, ro.get_columns_to_drop_3b, CONFIG_1["knot_spacing_3b"])):
        for r in values:
            try:
                fn(basis, r, spacing)
            except ValueError as exc:
                out["raises"][which][repr(r)] = str(exc)
            else:
                raise AssertionError(f"{which} at {r} did not raise")
    with open(os.path.join(HERE, "optimize_cases.json"), "w") as f:
        json.dump(out, f)
        f.write("\n")


if __name__ == "__main__":
    main()
