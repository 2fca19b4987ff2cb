"""Basis builders that both a device test and the host test of the basis plan (tests/test_basis_plan_host.py) use."""
import functools

import numpy as np

from uf3_amd.data import composition
from uf3_amd.representation import bspline

# the species sets of tests/test_gpu_species.py
ELEMENTS = {4: ['V', 'Nb', 'Mo', 'W'], 5: ['V', 'Nb', 'Mo', 'Ta', 'W'], 6: ['V', 'Cr', 'Nb', 'Mo', 'Ta', 'W'],
            8: ['H', 'C', 'Ni', 'Zr', 'Mo', 'W', 'Pt', 'U']}


def mixed_trio_basis(els, seed):
    """Every trio its own cut-offs and resolution (equal neighbour species: symmetric legs)."""
    rng = np.random.default_rng(seed)
    cs = composition.ChemicalSystem(els, 3)
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    rmax, res = {}, {}
    for t in trios:
        r1, l1 = float(rng.uniform(3.2, 4.0)), int(rng.integers(5, 8))
        r2, l2 = (r1, l1) if t[1] == t[2] else (float(rng.uniform(3.2, 4.0)), int(rng.integers(5, 8)))
        rmax[t] = [r1, r2, r1 + r2]
        res[t] = [l1, l2, int(rng.integers(9, 15))]
    return bspline.BSplineBasis(
        cs, r_min_map={**{p: 0.001 for p in pairs}, **{t: [1.5, 1.5, 1.5] for t in trios}},
        r_max_map={**{p: 5.5 for p in pairs}, **rmax}, resolution_map={**{p: 15 for p in pairs}, **res},
        leading_trim={2: 0, 3: 3}, trailing_trim={2: 3, 3: 3})


@functools.lru_cache(maxsize=None)
def wide_basis():
    """W with an untrimmed leading edge and a fine 3-body grid, built large on purpose: 16 rows of it do not fit the fused
    site-grade kernel's LDS (F > 608, the largest F whose tile fits 80 KB beside the index arrays)."""
    cs = composition.ChemicalSystem(["W"], 3)
    t = ("W", "W", "W")
    return bspline.BSplineBasis(cs, r_min_map={("W", "W"): 0.5, t: [1.0, 1.0, 1.0]}, r_max_map={("W", "W"): 5.0, t: [3.6, 3.6, 7.2]},
                                resolution_map={("W", "W"): 12, t: [10, 10, 18]}, leading_trim=0, trailing_trim=3)
