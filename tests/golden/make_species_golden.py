#!/usr/bin/env python3
"""
Golden capture beyond three species.  Runs ONLY in the build container, like make_golden.py (same stand-ins, reference at
/root/reference; nothing that travels to the GPU box imports this script):

    python tests/golden/make_species_golden.py

Two cases, written in make_golden.py's layout (inputs, meta, xe / xf, neighbour indices) so that _util.load_case reads them:

    case_bcc24_s4        24-atom rattled bcc cell of Cr / Mo / Ta / W, the notebook basis on every pair and trio
    case_bcc16_s8        16-atom rattled bcc cell, two atoms of each of H, C, Ni, Zr, Mo, W, Pt, U (Z = 1 ... 92), a basis of
                         coarser resolution (F = 8164; the notebook one would be 22 256 columns)
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
warnings.simplefilter("ignore")

import make_golden as mg  # noqa: E402  (puts the stand-ins and the reference on sys.path)

ase, rc = mg.ase, mg.rc

S4 = ['Cr', 'Mo', 'Ta', 'W']
S8 = ['H', 'C', 'Ni', 'Zr', 'Mo', 'W', 'Pt', 'U']


def kwargs(els, res2, res3, lead3):
    cs = rc.ChemicalSystem(els, 3)
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    return dict(r_min_map={**{p: 0.001 for p in pairs}, **{t: [1.5, 1.5, 1.5] for t in trios}},
                r_max_map={**{p: 5.5 for p in pairs}, **{t: [3.5, 3.5, 7.0] for t in trios}},
                resolution_map={**{p: res2 for p in pairs}, **{t: list(res3) for t in trios}},
                leading_trim={2: 0, 3: lead3}, trailing_trim={2: 3, 3: 3})


def main():
    rng = np.random.default_rng(4848)
    pos, cell = mg.bcc_cell(rng, (2, 2, 3))
    z4 = list(rng.permutation(np.repeat(S4, 6)))
    g4 = ase.Atoms(z4, positions=pos, pbc=True, cell=cell)
    mg.save_case("case_bcc24_s4", g4, S4, 3, kwargs(S4, 15, (6, 6, 12), 3))
    pos, cell = mg.bcc_cell(rng, (2, 2, 2), rattle=0.1)
    z8 = list(rng.permutation(np.repeat(S8, 2)))
    g8 = ase.Atoms(z8, positions=pos, pbc=True, cell=cell)
    mg.save_case("case_bcc16_s8", g8, S8, 3, kwargs(S8, 12, (5, 5, 10), 3))


if __name__ == "__main__":
    main()
