"""Bases whose l and m legs differ, the frames that go with them, and a census of what their leg masks do: shared by
tests/test_uneven_legs_host.py and tests/test_gpu_uneven_legs.py.

- ``uneven_basis``: every pair and every trio with ranges and resolutions of its own, l != m wherever the neighbour species
  differ (equal neighbour species: l = m, symmetry 2).  The l and m ranges of a trio are shorter than the 3-body list range (the
  largest of them all), so the per-trio masks of all three legs reject list entries.
- ``sym1_unary`` / ``sym1_binary``: equal neighbour species on unequal legs (symmetry 1).  Which of two equal-species neighbours
  takes leg l then decides the number: the neighbour with the lower reference supercell index as seen from the real copy of the
  centre.  The energy depends on the numbering of the atoms and on which cell image holds each, so the frames
  are given wrapped into their cell: the device and the references must see the same images.
- ``restated``: energy and forces of the triplet rule stated once more, with the two ways to get it wrong as variants."""
import functools
import json
import os

import numpy as np

from oracle import oracle as O
from uf3_amd import synthetic
from uf3_amd.data import composition
from uf3_amd.data.atoms import Atoms
from uf3_amd.representation import bspline
from _util import GOLDEN, basis_from_meta, wrapped
import _flux_ref as FR

UNEVEN_ELEMENTS = ["Nb", "Mo", "W"]
UNEVEN_NUMBERS = [41, 42, 74]


def uneven_basis(elements, seed, lead3):
    """Pairs: r_min 0.2-1.0, r_max 4.2-5.6, resolution 8-15.  Trio legs l, m: r_min 1.7-2.5, r_max 3.0-4.2, resolution 4-7, drawn
    per leg (once for both when the neighbour species are equal); leg n: r_min 1.6-2.6, r_max 0.7-0.9 of r_max_l + r_max_m,
    resolution 6-10.  Trailing trim 3, leading trim of the 3-body terms ``lead3``."""
    rng = np.random.default_rng(seed)
    cs = composition.ChemicalSystem(elements, 3)
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    rmin, rmax, res = {}, {}, {}
    for p in pairs:
        rmin[p], rmax[p], res[p] = float(rng.uniform(0.2, 1.0)), float(rng.uniform(4.2, 5.6)), int(rng.integers(8, 16))
    for t in trios:
        def leg():
            return float(rng.uniform(1.7, 2.5)), float(rng.uniform(3.0, 4.2)), int(rng.integers(4, 8))
        lo_l, hi_l, n_l = leg()
        lo_m, hi_m, n_m = (lo_l, hi_l, n_l) if t[1] == t[2] else leg()
        rmin[t] = [lo_l, lo_m, float(rng.uniform(1.6, 2.6))]
        rmax[t] = [hi_l, hi_m, float(rng.uniform(0.7, 0.9)) * (hi_l + hi_m)]
        res[t] = [n_l, n_m, int(rng.integers(6, 11))]
    return bspline.BSplineBasis(cs, r_min_map=rmin, r_max_map=rmax, resolution_map=res,
                                leading_trim={2: 0, 3: int(lead3)}, trailing_trim={2: 3, 3: 3})


def sym1_unary():
    """the basis of tests/golden/case_w16_sym1.npz: W, trio r_max [3.2, 3.8, 6.4], resolution [4, 5, 8], leading trim 0"""
    meta = json.loads(str(np.load(os.path.join(GOLDEN, "case_w16_sym1.npz"), allow_pickle=False)["meta"]))
    return basis_from_meta(meta)


def sym1_binary():
    """Mo / W, every trio at the settings of ``sym1_unary``: the trios with equal neighbour species have symmetry 1"""
    cs = composition.ChemicalSystem(["Mo", "W"], 3)
    pairs, trios = cs.interactions_map[2], cs.interactions_map[3]
    return bspline.BSplineBasis(
        cs, r_min_map={**{p: 0.5 for p in pairs}, **{t: [1.0, 1.0, 1.0] for t in trios}},
        r_max_map={**{p: 5.0 for p in pairs}, **{t: [3.2, 3.8, 6.4] for t in trios}},
        resolution_map={**{p: 10 for p in pairs}, **{t: [4, 5, 8] for t in trios}}, leading_trim=0, trailing_trim=3)


@functools.lru_cache(maxsize=None)
def basis(name):
    """"uneven_lead0", "uneven_lead3", "sym1_unary", "sym1_binary": one object per name (device tables hang on it)"""
    if name.startswith("uneven_lead"):
        return uneven_basis(UNEVEN_ELEMENTS, 2024, int(name[-1]))
    return {"sym1_unary": sym1_unary, "sym1_binary": sym1_binary}[name]()


BASES = ["uneven_lead0", "uneven_lead3", "sym1_unary", "sym1_binary"]


MODEL_SEED = 18       # (a draw under which the energy of every frame below feels the assignment: test_sensitivity asserts it)


def coefficients(b, seed=MODEL_SEED):
    """seeded model coefficients, the frozen ones zero (tests/test_gpu_virial.py::_model)"""
    coeff = np.random.default_rng(seed).normal(0, 0.05, b.n_feats)
    coeff[np.asarray(b.col_idx, dtype=int)] = 0.0
    return coeff


def _bcc(numbers, reps, a, seed, rattle):
    """rattled bcc, the species in equal shares and shuffled; the lattice sites a quarter of the lattice constant off the cell's
    faces, so that every atom lies inside the cell and stays there over a short walk"""
    base = synthetic.lattice_frame("bcc", reps, a, [numbers[0]], seed, rattle=rattle)
    z = np.random.default_rng(seed).permutation(np.resize(np.asarray(numbers), len(base)))
    return wrapped(Atoms(numbers=z, positions=base.get_positions() + 0.25 * a, cell=base.get_cell(), pbc=True))


def inside_cell(atoms):
    frac = np.asarray(atoms.get_positions(), dtype=float) @ np.linalg.inv(np.asarray(atoms.get_cell(), dtype=float))
    return bool(np.all(frac >= 0) and np.all(frac < 1))


@functools.lru_cache(maxsize=None)
def frames(name):
    """The ragged batch of a basis (16 to 36 atoms a frame).  Uneven: Nb / Mo / W at a lattice constant of 2.6 to 2.75 A, where the
    first shell (2.25 to 2.4 A +- rattle) straddles the legs' r_min.  Sym-1: 3.165 A, one frame a single cell thick (every atom
    neighbours its own images)."""
    if name.startswith("uneven"):
        return (_bcc(UNEVEN_NUMBERS, (2, 2, 3), 2.6, 11, 0.12), _bcc(UNEVEN_NUMBERS, (2, 2, 2), 2.7, 12, 0.12),
                _bcc(UNEVEN_NUMBERS, (3, 2, 3), 2.75, 13, 0.12))
    numbers = [74] if name == "sym1_unary" else [42, 74]
    return (_bcc(numbers, (2, 2, 2), 3.165, 21, 0.08), _bcc(numbers, (2, 2, 3), 3.165, 22, 0.08),
            _bcc(numbers, (3, 3, 1), 3.165, 23, 0.08))


@functools.lru_cache(maxsize=None)
def small_frame(name):
    """<= 16 atoms: differences of 3N force evaluations stay cheap"""
    if name.startswith("uneven"):
        return _bcc(UNEVEN_NUMBERS, (2, 2, 2), 2.65, 31, 0.12)
    return _bcc([74] if name == "sym1_unary" else [42, 74], (2, 2, 2), 3.165, 32, 0.08)


@functools.lru_cache(maxsize=None)
def mc_frame(name):
    """The frame of the Monte Carlo tests: enough atoms for 48 distinct transmutations (two species: one per atom)."""
    if name.startswith("uneven"):
        return frames(name)[0]
    return _bcc([74] if name == "sym1_unary" else [42, 74], (3, 3, 3), 3.165, 24, 0.08)


def all_frames(name):
    """every frame tests/test_gpu_uneven_legs.py puts on the device"""
    out = frames(name) + (small_frame(name),)
    return out if any(mc_frame(name) is a for a in out) else out + (mc_frame(name),)


def displaced(atoms, pos):
    return Atoms(numbers=atoms.get_atomic_numbers(), positions=pos, cell=atoms.get_cell(), pbc=atoms.get_pbc())


def with_numbers(atoms, z):
    return Atoms(numbers=np.asarray(z), positions=atoms.get_positions(), cell=atoms.get_cell(), pbc=atoms.get_pbc())


# ------------------------------------------------------------------------------------------------ the triplets of a frame
def _trio_tables(ob):
    tk, off = [], 0
    for t in range(len(ob.trios)):
        ks = []
        for q in range(3):
            nk = int(ob.trio_nk[t][q])
            ks.append(np.asarray(ob.trio_knots[off:off + nk]))
            off += nk
        tk.append(ks)
    rmin3 = min(k[0][0] for k in tk)
    rmax3 = max(max(k[0][-1], k[1][-1]) for k in tk)
    trio_of = {(int(zc), int(za), int(zb)): t for t, (zc, za, zb) in enumerate(ob.trio_z)}
    return tk, rmin3, rmax3, trio_of


def triplets(ob, atoms, variant=None):
    """Every candidate triplet of the frame: real centre i, unordered pairs of supercell atoms inside the 3-body list range
    (the oracle's, the largest l or m range), leg l on the lower atomic number and, for equal species, on the lower supercell
    index.  Yields (i, j, k, trio, leg vectors [3, 3], lengths [3], knots); j, k are supercell indices, parent = index % N.
    ``variant``: "exchange_lm" puts EVERY triplet's neighbours on the wrong legs, "reverse_equal" only those of equal species."""
    tk, rmin3, rmax3, trio_of = _trio_tables(ob)
    reach = max(float(np.max(ob.pair_rmax)), rmax3)
    sc_pos, sc_z, _ = O.supercell(atoms, 2.0 * reach)
    n = len(atoms.get_atomic_numbers())
    for i in range(n):
        d = sc_pos - sc_pos[i]
        r = np.linalg.norm(d, axis=1)
        zi = int(sc_z[i])
        nb = np.flatnonzero((r > rmin3) & (r <= rmax3))
        for x in range(len(nb)):
            for y in range(x + 1, len(nb)):
                j, k = int(nb[x]), int(nb[y])
                if sc_z[j] > sc_z[k]:
                    j, k = k, j
                t = trio_of.get((zi, int(sc_z[j]), int(sc_z[k])))
                if t is None:
                    continue
                if variant == "exchange_lm" or (variant == "reverse_equal" and sc_z[j] == sc_z[k]):
                    j, k = k, j
                dv = np.array([d[j], d[k], d[k] - d[j]])
                yield i, j, k, t, dv, np.linalg.norm(dv, axis=1), tk[t]


def leg_census(ob, atoms):
    """What the per-trio leg masks do to the triplets inside the list range: dict(accepted, l_lower, l_upper, m_lower, m_upper,
    n_lower, n_upper, ambiguous).  A triplet counts under every mask it fails.  ``ambiguous``: accepted triplets whose neighbours
    have one species while the trio's l and m legs differ and so do the two lengths: the other assignment is another number."""
    out = dict.fromkeys(("accepted", "l_lower", "l_upper", "m_lower", "m_upper", "n_lower", "n_upper", "ambiguous"), 0)
    sc_n = len(atoms.get_atomic_numbers())
    z = np.asarray(atoms.get_atomic_numbers())
    for i, j, k, t, dv, rr, ks in triplets(ob, atoms):
        ok = True
        for q, leg in enumerate("lmn"):
            if not rr[q] > ks[q][0]:
                out[leg + "_lower"] += 1
                ok = False
            if not rr[q] < ks[q][-1]:
                out[leg + "_upper"] += 1
                ok = False
        if ok:
            out["accepted"] += 1
            same_legs = len(ks[0]) == len(ks[1]) and np.array_equal(ks[0], ks[1])
            if z[j % sc_n] == z[k % sc_n] and not same_legs and abs(rr[0] - rr[1]) > 1e-6:
                out["ambiguous"] += 1
    return out


def restated(ob, atoms, coeff, variant=None):
    """(E, F [N, 3]) with the 3-body part over ``triplets(variant)``; the one- and two-body parts are _flux_ref's."""
    _, _, c3 = O.split_coefficients(ob, coeff)
    grids, off = [], 0
    for shp in ob.grid_shapes:
        size = int(np.prod(shp))
        grids.append(c3[off:off + size].reshape(shp))
        off += size
    n = len(atoms.get_atomic_numbers())
    one, tl = FR.terms(ob, atoms, coeff)
    E = float(one.sum())
    F = np.zeros((n, 3))
    for i, val, slots in tl:
        if len(slots) == 1:
            E += val
            for p, _, g in slots:
                F[p] -= g
                F[i] += g
    for i, j, k, t, dv, rr, ks in triplets(ob, atoms, variant):
        if not all(ks[q][0] < rr[q] < ks[q][-1] for q in range(3)):
            continue
        bv = [[FR._basis(ks[q], rr[q], nu)[0] for nu in range(2)] for q in range(3)]
        G = grids[t]
        E += float(np.einsum("abc,a,b,c->", G, bv[0][0], bv[1][0], bv[2][0]))
        g = np.array([np.einsum("abc,a,b,c->", G, bv[0][1], bv[1][0], bv[2][0]),
                      np.einsum("abc,a,b,c->", G, bv[0][0], bv[1][1], bv[2][0]),
                      np.einsum("abc,a,b,c->", G, bv[0][0], bv[1][0], bv[2][1])])
        u = dv / rr[:, None]
        gj, gk = g[0] * u[0] - g[2] * u[2], g[1] * u[1] + g[2] * u[2]
        F[j % n] -= gj
        F[k % n] -= gk
        F[i] += gj + gk
    return E, F
