"""Host site rows for tests/test_site_rows_host.py and tests/test_gpu_site_grade.py: B [N, F] with B[i] @ c = the site energy
U_i of _flux_ref.site_terms for every flat coefficient vector c.

By linearity and with no physics of its own: U_i = sum over the terms of i of (raw basis products) . (c1 | c2 | c3), and the
expanded model (c1 | c2 | c3) = E c is linear in the flat one.  The walk over the terms is _flux_ref.terms' (the same supercell,
the same ranges, the same leg rule: the lower atomic number, then the lower supercell index, takes leg l), keeping each term's
basis values instead of contracting them with one model; E comes from oracle.split_coefficients on the unit vectors -- the
fold and trim maps are the oracle's, not restated.  tests/test_site_rows_host.py holds B to _flux_ref.site_terms and to the
oracle's energy row."""
import functools

import numpy as np

from oracle import oracle as O
import _flux_ref as FR


def expansion(ob, n_feat):
    """E1 [S, F], E2 [len c2, F], E3 [len c3, F]: split_coefficients column by column."""
    cols = [O.split_coefficients(ob, e) for e in np.eye(n_feat)]
    return tuple(np.stack([np.asarray(c[q], dtype=float).reshape(-1) for c in cols], axis=1) for q in range(3))


def raw_rows(ob, atoms):
    """R1 [N, S], R2 [N, len c2], R3 [N, len c3]: every site energy's raw basis products (_flux_ref.terms' walk, values only)."""
    z = np.asarray(atoms.get_atomic_numbers())
    n = len(z)
    pair_rmax = np.asarray(ob.pair_rmax)
    tk, off = [], 0
    for t in range(len(ob.trios)):
        ks = []
        for q in range(3):
            nk = int(ob.trio_nk[t][q])
            ks.append(ob.trio_knots[off:off + nk])
            off += nk
        tk.append(ks)
    rmin3 = rmax3 = 0.0
    if tk:
        rmin3 = min(k[0][0] for k in tk)
        rmax3 = max(max(k[0][-1], k[1][-1]) for k in tk)
    reach = max(pair_rmax.max(), rmax3)
    sc_pos, sc_z, _ = O.supercell(atoms, 2.0 * reach)
    zs = [int(q) for q in ob.species_z]
    pk, p_off, kp, cp = [], [], 0, 0
    for p in range(len(ob.pairs)):
        nk = int(ob.pair_nk[p])
        pk.append(ob.pair_knots[kp:kp + nk]); p_off.append(cp)
        kp += nk; cp += nk - 4
    pair_of = {}
    for p, (za, zb) in enumerate(ob.pair_z):
        pair_of[(int(za), int(zb))] = p; pair_of[(int(zb), int(za))] = p
    trio_of = {(int(zc), int(za), int(zb)): t for t, (zc, za, zb) in enumerate(ob.trio_z)}
    t_off, o3 = [], 0
    for shp in ob.grid_shapes:
        t_off.append(o3); o3 += int(np.prod(shp))
    R1, R2, R3 = np.zeros((n, len(zs))), np.zeros((n, cp)), np.zeros((n, o3))
    for i in range(n):
        R1[i, zs.index(int(z[i]))] = 1.0
        d = sc_pos - sc_pos[i]
        r = np.linalg.norm(d, axis=1)
        zi = int(sc_z[i])
        for j in np.flatnonzero(r > 0):
            p = pair_of.get((zi, int(sc_z[j])))
            if p is None:
                continue
            if not (max(float(ob.pair_rmin[p]), 0.0) < r[j] < pair_rmax[p]):
                continue
            v = np.nan_to_num(FR._basis(pk[p], r[j], 0)[0])
            R2[i, p_off[p]:p_off[p] + len(v)] += v
        if not tk:
            continue
        nb = np.flatnonzero((r > rmin3) & (r <= rmax3))
        for x in range(len(nb)):
            for y in range(x + 1, len(nb)):
                j, k = nb[x], nb[y]
                if sc_z[j] > sc_z[k]:
                    j, k = k, j
                t = trio_of.get((zi, int(sc_z[j]), int(sc_z[k])))
                if t is None:
                    continue
                rr = np.linalg.norm(np.array([d[j], d[k], d[k] - d[j]]), axis=1)
                if not all(tk[t][q][0] < rr[q] < tk[t][q][-1] for q in range(3)):
                    continue
                bv = [np.nan_to_num(FR._basis(tk[t][q], rr[q], 0)[0]) for q in range(3)]
                size = int(np.prod(ob.grid_shapes[t]))
                R3[i, t_off[t]:t_off[t] + size] += np.einsum("a,b,c->abc", *bv).reshape(-1)
    return R1, R2, R3


def site_rows(ob, atoms, n_feat):
    """B [N, F]."""
    E1, E2, E3 = _expansion_cached(ob, n_feat)
    R1, R2, R3 = raw_rows(ob, atoms)
    B = R1 @ E1
    if E2.size:
        B = B + R2 @ E2
    if E3.size:
        B = B + R3 @ E3
    return B


@functools.lru_cache(maxsize=None)
def _expansion_cached(ob, n_feat):
    return expansion(ob, n_feat)


# ------------------------------------------------------------------------------------------------ shared fixtures
def seeded_model(basis, seed=5):
    """A model with a posterior on ``basis``: tests/test_leverage_host.py::fixture_model's recipe (Gram pieces -> fit_with_gram)
    with seeded sparse rows in place of the golden file's."""
    from uf3_amd.regression import least_squares as ls
    model = ls.WeightedLinearModel(basis)
    rng = np.random.default_rng(seed)
    F, mask = model.n_feats, np.asarray(model.mask)
    x = rng.normal(0, 1, (3 * F, F)) * (rng.random((3 * F, F)) < 0.3)
    y = rng.normal(0, 1, 3 * F)
    model.fit_with_gram(x[:, mask].T @ x[:, mask], x[:, mask].T @ y)
    return model


@functools.lru_cache(maxsize=None)
def case(name):
    """(basis, frame): "unary" W 16 atoms on tests/golden/model_unary.json's basis, "mow" Mo/W 16 atoms on the notebook basis
    (3-body terms on every trio), "uneven" Nb/Mo/W on _uneven's lead-0 basis (l != m legs, per-trio ranges), "sym1" W on the
    symmetry-1 basis (the supercell-index tie-break decides the column), "cluster" 13 W atoms without a cell, "pairs" the unary
    frame on a 2-body-only basis."""
    import os
    from uf3_amd import synthetic
    from uf3_amd.data import composition
    from uf3_amd.data.atoms import Atoms
    from uf3_amd.regression import least_squares as ls
    from uf3_amd.representation import bspline
    from _util import GOLDEN
    import _uneven
    unary = ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json")).bspline_config
    w16 = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=3)
    if name == "unary":
        return unary, w16
    if name == "mow":
        return synthetic.notebook_basis(["Mo", "W"]), synthetic.lattice_frame("bcc", (2, 2, 2), 3.2, [42, 74], seed=5)
    # (_uneven's settings on objects of this module's own: device tables hang on a basis object, and _uneven.basis' cached ones
    # belong to the tests that make their own contexts for them)
    if name == "uneven":
        return _uneven.uneven_basis(_uneven.UNEVEN_ELEMENTS, 2024, 0), _uneven.small_frame("uneven_lead0")
    if name == "sym1":
        return _uneven.sym1_unary(), _uneven.small_frame("sym1_unary")
    if name == "cluster":
        pos = np.asarray(synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=7).get_positions(), dtype=float)
        keep = np.sort(np.argsort(np.linalg.norm(pos - pos.mean(axis=0), axis=1))[:13])
        return unary, Atoms(numbers=np.full(13, 74), positions=pos[keep], cell=np.zeros((3, 3)), pbc=False)
    if name == "pairs":
        cs = composition.ChemicalSystem(["W"], 2)
        return bspline.BSplineBasis(cs, r_min_map={("W", "W"): 0.5}, r_max_map={("W", "W"): 5.0}, resolution_map={("W", "W"): 12},
                                    leading_trim=0, trailing_trim=3), w16
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """Host B of a case: computed once, shared, never changed."""
    basis, atoms = case(name)
    B = site_rows(O.OracleBasis(basis), atoms, basis.n_feats)
    B.setflags(write=False)
    return B
