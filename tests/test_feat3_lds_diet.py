"""
k_featurize3's neighbour role keeps the headers of its staged records (fixed bond, first n slot) in registers: a lane per
slot of the pass, two records' slots per scalar read.  Force rows against the oracle on cells whose
neighbour roles stage 0, 1, exactly NREC, NREC + 1 and several times NREC valid records, at list capacities 16 and 24 and on
sparse cells; and nothing may outlive a pass: a frame featurized alone and as the last frame of a batch gives the same force
rows bit for bit.

Tolerance: that of the three-way test of the trio kernels (test_gpu_parity.py), 1e-9 relative against the oracle.
"""
import itertools

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic, _lib
from uf3_amd.representation import process
from _util import rel_err

pytestmark = pytest.mark.gpu
TOL = 1e-9
NREC = 29           # neighbour-role records per engine pass of the 3-row window (F3Cfg<3, 1>::NREC, uf3_feat3.h)
R_MIN = 1.5         # lower end of every 3-body leg of the bases below


def _basis(elements, r3):
    """The notebook basis (3 x 3 x 9 kept bins per trio) with the centre legs cut at ``r3``."""
    cs = synthetic.composition.ChemicalSystem(list(elements), 3)
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    return synthetic.bspline.BSplineBasis(
        cs, r_min_map={**{p: 0.001 for p in pairs}, **{t: [R_MIN, R_MIN, R_MIN] for t in trios}},
        r_max_map={**{p: 5.5 for p in pairs}, **{t: [r3, r3, 2 * r3] for t in trios}},
        resolution_map={**{p: 15 for p in pairs}, **{t: [6, 6, 12] for t in trios}}, leading_trim={2: 0, 3: 3}, trailing_trim={2: 3, 3: 3})


def _role_records(atoms, r3):
    """Valid records of every neighbour role, from the geometry alone: for atom m, centre species sc and partner species sx
    the pairs (e, k) with e a 3-body neighbour of m of species sc, k one of e of species sx, k not m itself and |m -> k| inside
    leg n.  The open intervals (R_MIN, r3) and (R_MIN, 2 r3) are the kernel's (t0, tlast) of the legs: the trims of ``_basis`` drop
    basis functions, they do not move the ends of a leg's knot sequence.  Returns ({(m, sc, sx): count}, 3-body list length of
    every atom)."""
    pos = np.asarray(atoms.get_positions(), float)
    cell = np.asarray(atoms.get_cell(), float).reshape(3, 3)
    z = np.asarray(atoms.get_atomic_numbers())
    n = len(z)
    span = [int(np.ceil(r3 * np.linalg.norm(np.linalg.inv(cell)[:, k]))) for k in range(3)]
    shifts = np.array(list(itertools.product(*[range(-s, s + 1) for s in span]))) @ cell
    lists = []
    for m in range(n):
        d = (pos[None, :, :] + shifts[:, None, :] - pos[m]).reshape(-1, 3)
        r = np.linalg.norm(d, axis=1)
        keep = np.flatnonzero((r > R_MIN) & (r < r3))
        lists.append((keep % n, d[keep]))
    counts = {}
    for m in range(n):
        for sc in np.unique(z):
            for sx in np.unique(z):
                c = 0
                for e, de in zip(*lists[m]):
                    if z[e] != sc:
                        continue
                    k, dk = lists[e]
                    rn = np.linalg.norm(de + dk, axis=1)          # 0 where k is m itself
                    c += int(np.count_nonzero((z[k] == sx) & (rn > R_MIN) & (rn < 2 * r3)))
                counts[(m, int(sc), int(sx))] = c
    return counts, np.array([len(l[0]) for l in lists])


SEVERAL = "several"            # a role of at least three full passes
# (name, lattice, repetitions, lattice constant, atomic numbers, seed, cut-off of the centre legs, longest list, what its roles hold)
CELLS = [
    ("w_cap16", "bcc", (2, 2, 2), 3.165, [74], 300, 3.5, 14, {SEVERAL}),
    ("mow_cap16", "bcc", (3, 3, 3), 3.165, [42, 74], 300, 3.5, 14, {NREC, NREC + 1, SEVERAL}),
    ("nbmow_cap16", "bcc", (3, 3, 3), 3.165, [41, 42, 74], 300, 3.5, 14, {0, 1, NREC, NREC + 1}),
    ("w_cap24", "fcc", (2, 2, 2), 3.9, [74], 300, 4.0, 18, {SEVERAL}),
    ("mow_cap24", "fcc", (2, 2, 3), 3.9, [42, 74], 301, 4.0, 18, {NREC, NREC + 1, SEVERAL}),
    ("nbmow_cap24", "fcc", (2, 2, 3), 3.9, [41, 42, 74], 300, 4.0, 18, {NREC, NREC + 1, SEVERAL}),
    ("nbmow_cap24_rare", "fcc", (2, 2, 3), 3.9, [41, 42, 74], 321, 4.0, 18, {0, 1, SEVERAL}),
    ("w_sparse", "bcc", (2, 2, 2), 4.0, [74], 302, 3.5, 8, {NREC, NREC + 1}),
    ("nbmow_sparse", "bcc", (3, 3, 3), 3.9, [41, 42, 74], 300, 3.5, 8, {0, 1}),
]
ELEMENTS = {74: "W", 42: "Mo", 41: "Nb"}


@pytest.mark.parametrize("name,lattice,reps,a,numbers,seed,r3,longest,want", CELLS, ids=[c[0] for c in CELLS])
def test_neighbour_role_record_counts_against_oracle(name, lattice, reps, a, numbers, seed, r3, longest, want, monkeypatch, capfd):
    atoms = synthetic.lattice_frame(lattice, reps, a, numbers, seed=seed, rattle=0.03, strain=0.0)
    basis = _basis([ELEMENTS[z] for z in sorted(numbers)], r3)
    monkeypatch.setenv("UF3_DEBUG_LDS", "1")                      # (read when the context is made: the launches say what they are)
    monkeypatch.setattr(_lib, "_contexts", {})                    # (a context of its own: capacities are a context's grow-only memory)
    fz = process.BasisFeaturizer(basis)
    assert fz._dev()[1].featurizer_modes & 0x1000                 # the bond-factorised launch serves this basis
    # the cases this cell is here for occur: role counts from the geometry, tied to the lists the launches consumed
    counts, lengths = _role_records(atoms, r3)
    ij = fz.product_n3_indices(atoms)
    assert np.array_equal(np.bincount(ij[:, 0], minlength=len(atoms)), lengths) and lengths.max() == longest
    have = set(counts.values())
    if max(have) >= 3 * NREC:
        have.add(SEVERAL)
    assert want <= have, (want, sorted(v for v in have if v != SEVERAL))
    ref = O.featurize(O.OracleBasis(basis), atoms)
    # the context's first force call runs the generic instance at the estimated capacity, the next one at the tuned capacity
    for call in range(2):
        capfd.readouterr()
        x_e, x_f, _ = fz.featurize_frames([atoms])
        said = capfd.readouterr().err
        err_e, err_f = rel_err(x_e[0], ref["xe"]), rel_err(x_f.reshape(ref["xf"].shape), ref["xf"])
        assert err_e < TOL and err_f < TOL, (call, err_e, err_f)
    if longest > 8:                                               # the instance laid out for 16 or 24 entries ran last
        assert f"uf3 featurize3: " in said and f", cap {(longest + 7) // 8 * 8} (lists" in said, said
    _lib.drop_device_basis(basis)


@pytest.mark.parametrize("lattice,reps,a,numbers,r3", [("bcc", (3, 3, 3), 3.165, [42, 74], 3.5), ("fcc", (2, 2, 3), 3.9, [41, 42, 74], 4.0)],
                         ids=["mow_cap16", "nbmow_cap24"])
def test_frame_alone_and_as_last_of_a_batch_bit_for_bit(lattice, reps, a, numbers, r3, monkeypatch):
    """Nothing is carried over between atoms, blocks or roles: the last frame's force rows do not depend on what ran before."""
    frames = [synthetic.lattice_frame(lattice, reps, a, numbers, seed=310 + k, rattle=0.03, strain=0.0) for k in range(4)]
    basis = _basis([ELEMENTS[z] for z in sorted(numbers)], r3)
    monkeypatch.setattr(_lib, "_contexts", {})
    fz = process.BasisFeaturizer(basis)
    assert fz._dev()[1].featurizer_modes & 0x1000
    fz.featurize_frames(frames)                                   # (the capacity settles)
    _, xf_batch, off = fz.featurize_frames(frames)
    _, xf_alone, _ = fz.featurize_frames(frames[-1:])
    last = np.ascontiguousarray(xf_batch[off[-2]:off[-1]])
    assert last.shape == xf_alone.shape and np.abs(xf_alone).max() > 0
    assert np.array_equal(last.view(np.uint64), np.ascontiguousarray(xf_alone).view(np.uint64))
    _lib.drop_device_basis(basis)
