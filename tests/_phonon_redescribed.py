"""What tests/test_phonon_redescribed_host.py and tests/test_gpu_phonon_redescribed.py share: the frames and their descriptions
(tests/_util.py: Description), and how a phonon calculation on a description maps back to the base's.

A description B of a base frame A has the cell ``C_B = M C_A Q^T`` (M integer, |det M| = ``scale``) and atom k an image of A's atom
``src[k]``.  With n_super n_A on the base and n_B on the description the two supercells are the same physical crystal exactly when
``n_B C_B`` and ``n_A C_A Q^T`` span one lattice (``same_supercell``); then

- a wave vector keeps its Cartesian components, turned by Q: ``map_q``; with ``scale`` > 1 the ``scale`` wave vectors of the base
  that differ by a reciprocal vector of B's lattice fold onto one q of B (``fold_q``), and B's 3 N_B eigenvalues there are the
  sorted union of the base's at those;
- B's supercell atom p', seen from its home-cell atom i', is the base's supercell atom p seen from ``src[i']`` at the same
  separation modulo the supercell lattice (``pair_map``), so that ``fc_B[i', p'] = Q fc_A[src[i'], p] Q^T`` (``mapped_rows``).

``synthetic_rows`` is a short-ranged force-constant function of the separation vector alone, summed over the images of the
physical supercell in a way that does not look at how the cell is described; ``brute_force_images`` is the nearest-image search
by exhaustion; ``legacy_nearest_images`` the +-2 search this project used to have."""
import functools
import itertools

import numpy as np

from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import harmonic
from _util import SKEW_U, Description, describe, equivalence_cases, rotation
import test_redescribed_host as RH

A_W = 3.165
SHEAR = [[1, 0, 0], [1, 1, 0], [0, 1, 1]]          # a unimodular re-description that leaves a cubic cell compact
MAX_SUPERCELL = 130                                # atoms
TURN = rotation([1, 2, 3], 0.7)


def skew3():
    """The 3-atom triclinic Mo W2 cell of tests/test_gpu_phonon.py (_skew3)."""
    cell = np.array([[3.2, 0.0, 0.0], [0.5, 3.3, 0.0], [0.4, 0.6, 4.9]])
    frac = np.array([[0.02, 0.05, 0.01], [0.48, 0.53, 0.34], [0.55, 0.41, 0.69]])
    return Atoms(numbers=[42, 74, 74], positions=frac @ cell, cell=cell, pbc=True)


def conv2():
    """The 2-atom conventional bcc W cell, both atoms off their sites: no degenerate modes, nothing on a cell face."""
    frac = np.array([[0.11, 0.07, 0.05], [0.62, 0.55, 0.58]])
    return Atoms(numbers=[74, 74], positions=frac * A_W, cell=np.eye(3) * A_W, pbc=True)


def conv16():
    """The unrattled 2 x 2 x 2 conventional bcc W cell, 16 atoms: exact degeneracies at 3N = 48."""
    grid = np.array(list(np.ndindex(2, 2, 2)), dtype=float)
    pos = ((grid[:, None, :] + np.array([[0, 0, 0], [0.5, 0.5, 0.5]])[None]) * A_W).reshape(-1, 3)
    return Atoms(numbers=[74] * 16, positions=pos, cell=np.eye(3) * 2 * A_W, pbc=True)


@functools.lru_cache(maxsize=None)
def frames():
    """name -> (base frame, {label: Description}, model key: the case of ``test_redescribed_host.model`` or "unary")"""
    eq = equivalence_cases()
    mow, prim = eq["bcc_mow"][1], eq["bcc_w_primitive"][1]
    by = lambda case, names: {d.label: d for d in eq[case][2] if d.label in names}          # noqa: E731
    s3, c2 = skew3(), conv2()
    outside = RH.unwrapped_frames()["every_atom"][1]
    return {
        "bcc_mow": (mow, by("bcc_mow", ("skew_821", "skew_351", "skew_751", "perm_rotation_shift", "skew_751_reflection")),
                    "bcc_mow"),
        "bcc_w_primitive": (prim, {**by("bcc_w_primitive", ("skew_rotation",)),
                                   "folded_222": describe(prim, "folded_222", reps=(2, 2, 2)),
                                   "shear_rotation": describe(prim, "shear_rotation", U=SHEAR, Q=TURN)}, "unary"),
        "mow_skew3": (s3, {"skew_821": describe(s3, "skew_821", U=SKEW_U["skew_821"])}, "bcc_mow"),
        "w_conv2": (c2, {"skew_821": describe(c2, "skew_821", U=SKEW_U["skew_821"]),
                         "shear": describe(c2, "shear", U=SHEAR)}, "unary"),
        "bcc_mow_unwrapped": (mow, {"every_atom": Description("every_atom", outside, np.arange(len(mow)), 1, np.eye(3))},
                              "bcc_mow"),
    }


# the descriptions whose cells are as compact as the base's: the +-2 search was right on them
COMPACT = [("bcc_mow", "perm_rotation_shift"), ("bcc_w_primitive", "folded_222"), ("bcc_w_primitive", "shear_rotation"),
           ("w_conv2", "shear")]
SKEWS = [("bcc_mow", "skew_821"), ("bcc_mow", "skew_351"), ("bcc_mow", "skew_751")]


def base(frame):
    return frames()[frame][0]


def description(frame, label):
    return frames()[frame][1][label]


def n_super_pairs(frame, label):
    """(n_A, n_B) with n_B in 1, 2, 3, both supercells one physical crystal of 2 to MAX_SUPERCELL atoms (a supercell of one atom
    has no force constants left after the sum rule)"""
    a, d = base(frame), description(frame, label)
    out = []
    for nb in (1, 2, 3):
        na = nb * int(round(d.scale ** (1.0 / 3.0)))
        if 2 <= len(d.atoms) * nb ** 3 <= MAX_SUPERCELL and same_supercell(a, na, d, nb):
            out.append((na, nb))
    return out


def all_pairs(only=None):
    """[(frame, label, n_A, n_B)] over every description (or those of ``only``)"""
    return [(f, lab, na, nb) for f, (_, descs, _) in frames().items() for lab in descs
            if only is None or (f, lab) in only for na, nb in n_super_pairs(f, lab)]


def masses(atoms):
    return RH.masses(atoms)


def _cell(atoms):
    return np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)


def _unimodular(T, tol=1e-9):
    R = np.rint(T)
    return bool(np.abs(T - R).max() <= tol and abs(round(np.linalg.det(R))) == 1)


def generates(basis, lattice):
    """Do the rows of ``basis`` generate the lattice of the rows of ``lattice`` (and nothing more)?"""
    return _unimodular(np.asarray(lattice, float) @ np.linalg.inv(np.asarray(basis, float)))


def compact_supercell_basis(a, n_a, d):
    """The base's own supercell rows turned into the description's frame: the fixed compact basis of the physical supercell."""
    return n_a * _cell(a) @ d.Q.T


def same_supercell(a, n_a, d, n_b):
    return generates(compact_supercell_basis(a, n_a, d), n_b * _cell(d.atoms))


def map_q(a, d, q_b):
    """Reduced q of the base for reduced q of the description: the same Cartesian wave vector, turned back by Q."""
    k_b = np.atleast_2d(np.asarray(q_b, float)) @ np.linalg.inv(_cell(d.atoms)).T
    return (k_b @ d.Q) @ _cell(a).T


def fold_q(a, d, q_b):
    """[nq, scale, 3]: the base's wave vectors that fold onto each q of the description, ``map_q`` plus the reciprocal vectors of
    the description's lattice that are distinct modulo the base's: g M^-T with C_B Q = M C_A."""
    q0 = map_q(a, d, q_b)
    if d.scale == 1:
        return q0[:, None, :]
    M = np.rint(_cell(d.atoms) @ d.Q @ np.linalg.inv(_cell(a)))
    assert np.abs(M @ _cell(a) - _cell(d.atoms) @ d.Q).max() <= 1e-9
    span = int(np.abs(M).sum(axis=1).max())
    g = np.array(list(itertools.product(range(span + 1), repeat=3)), dtype=float) @ np.linalg.inv(M).T
    g = np.round(g - np.floor(g + 1e-9), 9)
    g = np.unique(np.where(g >= 1.0, 0.0, g), axis=0)
    assert len(g) == d.scale, (len(g), d.scale)
    return q0[:, None, :] + g[None, :, :]


def supercell_positions(atoms, n_super):
    return np.asarray(harmonic.supercell(atoms, n_super).get_positions(), dtype=float)


def pair_map(a, n_a, d, n_b, tol=1e-6):
    """int [N_B, N_sc]: ``pair_map[i', p']`` is the base's supercell atom p whose separation from atom ``src[i']`` is, modulo the
    supercell lattice, the description's p' from i' turned back by Q.  Every row is a bijection."""
    assert same_supercell(a, n_a, d, n_b)
    xa, xb = supercell_positions(a, n_a), supercell_positions(d.atoms, n_b) @ d.Q
    assert len(xa) == len(xb)
    inv = np.linalg.inv(n_a * _cell(a))
    out = np.empty((len(d.atoms), len(xb)), dtype=np.int64)
    for i in range(len(d.atoms)):
        sep_b = xb - xb[i]
        sep_a = xa - xa[d.src[i]]
        f = (sep_b[:, None, :] - sep_a[None, :, :]) @ inv
        hit = np.abs(f - np.rint(f)).max(axis=-1) <= tol
        assert np.all(hit.sum(axis=1) == 1) and np.all(hit.sum(axis=0) == 1), (d.label, i)
        out[i] = np.argmax(hit, axis=1)
    return out


def mapped_rows(fc_a, a, n_a, d, n_b):
    """fc_B[i', p'] = Q fc_A[src[i'], pair_map[i', p']] Q^T"""
    pm = pair_map(a, n_a, d, n_b)
    picked = np.asarray(fc_a)[d.src[:len(d.atoms), None], pm]
    return np.einsum("ab,ipbc,dc->ipad", d.Q, picked, d.Q)


def spectrum_scale(lam, q):
    """What an eigenvalue deviation at each q is relative to: max |lam| of that q -- but of all the q at an integer q, where D
    of a one-atom cell vanishes by the sum rule and what is left of it is the rounding of a sum of terms of the spectrum's size."""
    lam, q = np.asarray(lam), np.atleast_2d(q)
    scale = np.abs(lam).max(axis=1)
    return np.where(np.all(q == np.rint(q), axis=1), np.abs(lam).max(), scale)


def folded_union(lam_a):
    """lam [nq, scale, 3 N_A] -> [nq, scale 3 N_A] ascending: the description's eigenvalues at the folded q"""
    lam_a = np.asarray(lam_a)
    return np.sort(lam_a.reshape(lam_a.shape[0], -1), axis=1)


# ---- a synthetic force-constant function ---------------------------------------------------------------------------------------
RANGE = 6.0                        # Angstrom
STRENGTH = {42: 1.0, 74: 1.3}


def pair_block(r, ci, cj):
    """Phi(r) [..., 3, 3] = -c_i c_j g(|r|) (3 r r^T / r^2 + I / 2), g = 5 (1 - (r / RANGE)^2)^3 inside RANGE and 0 outside,
    0 at r = 0: covariant, Phi(Q r) = Q Phi(r) Q^T."""
    r = np.asarray(r, float)
    d2 = (r * r).sum(axis=-1)
    inside = (d2 < RANGE * RANGE) & (d2 > 1e-12)
    g = np.where(inside, 5.0 * (1.0 - d2 / RANGE ** 2) ** 3, 0.0) * ci * cj
    rr = r[..., :, None] * r[..., None, :] / np.where(inside, d2, 1.0)[..., None, None]
    return -g[..., None, None] * (3.0 * rr + 0.5 * np.eye(3))


def synthetic_rows(atoms, n_super, basis):
    """fc [N, N_sc, 3, 3] of ``pair_block`` on the n_super^3 supercell: every pair's images summed over the supercell lattice,
    found by reducing the separation against ``basis`` -- rows that generate that lattice, asserted, and that do not depend on
    how ``atoms`` describes the crystal -- then the acoustic sum rule on the self term."""
    basis = np.asarray(basis, float)
    assert generates(basis, n_super * _cell(atoms))
    inv = np.linalg.inv(basis)
    reach = np.ceil(RANGE * np.sqrt((inv * inv).sum(axis=0)) + 0.5).astype(int)
    ks = np.array(list(itertools.product(*(range(-m, m + 1) for m in reach))), dtype=float)
    x = supercell_positions(atoms, n_super)
    n = len(atoms)
    c = np.array([STRENGTH[int(z)] for z in harmonic.supercell(atoms, n_super).get_atomic_numbers()])
    fc = np.zeros((n, len(x), 3, 3))
    for i in range(n):
        f = (x - x[i]) @ inv
        f -= np.floor(f + 0.5)
        r = (f[:, None, :] + ks[None, :, :]) @ basis
        fc[i] = pair_block(r, c[i], c[:, None]).sum(axis=1)
        fc[i, i] -= fc[i].sum(axis=0)
    return fc


def host_eigenvalues(fc, atoms, q, n_super):
    return np.linalg.eigvalsh(harmonic.dynamical_matrices(fc, atoms, q, n_super, masses(atoms)))


# ---- the nearest images, by exhaustion and as they used to be searched ----------------------------------------------------------
def brute_force_images(atoms, n_super, compact, tol=1e-5):
    """``(terms int64 [m, 5], weights [m], worst)`` in ``harmonic.image_terms``'s layout and order, from a search over every
    translation of the supercell that can matter: ``compact`` generates the supercell lattice, so every point is within rho =
    (|c_1| + |c_2| + |c_3|) / 2 of a lattice point (half its cell's diagonal, at most), the nearest image of a pair is no farther
    than rho, and an image within rho + tol has |coefficient + fraction| <= (rho + tol) / h_a along the described supercell's
    row a, h_a its plane spacing.  ``worst`` is the largest nearest distance found over rho: <= 1 says the range sufficed."""
    cell, pos = _cell(atoms), np.asarray(atoms.get_positions(), float)
    sup = n_super * cell
    assert generates(compact, sup)
    rho = 0.5 * np.sqrt((np.asarray(compact, float) ** 2).sum(axis=1)).sum()
    inv = np.linalg.inv(sup)
    reach = (rho + tol) * np.sqrt((inv * inv).sum(axis=0)) * (1 + 1e-9)
    shifts = np.array(list(itertools.product(range(n_super), repeat=3)), dtype=np.int64)
    n = len(pos)
    terms, weights, worst = [], [], 0.0
    for i in range(n):
        for t, s in enumerate(shifts):
            for j in range(n):
                v = (s.astype(float) @ cell + pos[j]) - pos[i]
                f = v @ inv
                lo, hi = np.ceil(-reach - f).astype(int), np.floor(reach - f).astype(int)
                K = np.indices(tuple(hi - lo + 1)).reshape(3, -1).T + lo          # every triple of the box, in its order
                dist = np.sqrt(((v + K.astype(float) @ sup) ** 2).sum(axis=1))
                worst = max(worst, dist.min() / rho)
                near = K[dist <= dist.min() + tol]
                for k in near:
                    terms.append([i, t * n + j, *(s + n_super * k)])
                    weights.append(1.0 / len(near))
    return np.array(terms, dtype=np.int64), np.array(weights), worst


def legacy_nearest_images(sup, v, tol=1e-5):
    """``harmonic.nearest_images`` as the search used to be: the 125 translations (-2 .. 2)^3 of the basis as given."""
    sup, v = np.asarray(sup, float).reshape(3, 3), np.asarray(v, float).reshape(-1, 3)
    around = np.array(list(itertools.product((-2, -1, 0, 1, 2), repeat=3)), dtype=np.int64)
    w = v[:, None, :] + (around.astype(float) @ sup)[None, :, :]
    d = np.sqrt((w * w).sum(axis=-1))
    near = d <= d.min(axis=-1, keepdims=True) + tol
    pair, k = np.nonzero(near)
    return pair, around[k], near.sum(axis=-1), np.full(len(v), 125, dtype=np.int64)
