"""NumPy restatement of the image dependent pair potential on the device (uf3_amd/csrc/uf3_idpp.h; Smidstrup et al., J. Chem.
Phys. 140, 214106): the nearest-image vector, S and F of one image in float64 with the kernel's formulas and in ``np.longdouble``
(the yardstick of the device comparison), the ``_neb_ref.Band`` whose energies and forces they are, and the bands the host and
device tests share.  For tests/test_idpp_host.py and tests/test_gpu_idpp.py.

For image k of a band of M images, lambda = k / (M - 1):
    d_ij = |D_ij|, D_ij the nearest-image vector x_j - x_i;   t_ij = (1 - lambda) d_ij(R^0) + lambda d_ij(R^{M-1})
    S = sum_{i<j} (t_ij - d_ij)^2 / d_ij^4;   F_i = sum_{j != i} c_ij D_ij / d_ij,  c_ij = -2 (t - d) (d + 2 (t - d)) / d^5
Nearest-image vector: the fractional difference along the periodic axes (the cell completed for the others as ``neb._axes`` does)
has its rounding subtracted, as lattice vectors; among the 3^p shifts in {-1, 0, 1} on the p periodic axes around that result the
shortest vector is taken, ties to the first in the order s_a, s_b, s_c = -1, 0, 1 with s_c running fastest.  Periodic rows that
are mutually orthogonal (exact zeros) skip the search."""
import functools
import itertools

import numpy as np

from uf3_amd import synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import neb
import _neb_ref as N

SKEW = np.array([[1, 0, 0], [1, 1, 0], [0, 1, 1]])      # cell' = SKEW @ cell: the skewed re-description of the issue
A0_W = 3.17352


def completed(cell, pbc):
    """``neb._axes``, restated: rows of non-periodic axes replaced by unit vectors orthogonal to the rows already there."""
    full = np.array(cell, dtype=float).reshape(3, 3)
    pbc = np.asarray(pbc, bool).reshape(3)
    full[~pbc] = 0.0
    for k in np.flatnonzero(~pbc):
        full[k] = np.linalg.svd(full)[2][-1]
    return full


def _inverse(h):
    """The inverse of a 3 x 3 matrix by cofactors, in h's own dtype (np.linalg.inv has no longdouble)."""
    co = np.array([np.cross(h[1], h[2]), np.cross(h[2], h[0]), np.cross(h[0], h[1])])
    return co.T / np.dot(h[0], co[0])


def orthogonal(cell, pbc):
    cell = np.asarray(cell, float).reshape(3, 3)
    per = np.flatnonzero(np.asarray(pbc, bool).reshape(3))
    return all(np.dot(cell[a], cell[b]) == 0.0 for a, b in itertools.combinations(per, 2))


def nearest(D, cell, pbc, dtype=np.float64):
    """The nearest-image vectors of the differences ``D`` [..., 3] (module text), in ``dtype``."""
    pbc = np.asarray(pbc, bool).reshape(3)
    D = np.asarray(D, dtype=dtype)
    if not pbc.any():
        return D
    h = np.asarray(cell, dtype=float).reshape(3, 3).astype(dtype)
    inv = _inverse(completed(cell, pbc).astype(dtype))
    for k in np.flatnonzero(pbc):
        n = np.rint(D @ inv[:, k])                                       # (half to even, as the kernel's rint)
        D = D - n[..., None] * h[k]
    if orthogonal(cell, pbc):
        return D
    best = np.full(D.shape[:-1], np.inf, dtype=dtype)
    out = D.copy()
    rng = [(-1, 0, 1) if p else (0,) for p in pbc]
    for sa in rng[0]:
        va = D + dtype(sa) * h[0]
        for sb in rng[1]:
            vb = va + dtype(sb) * h[1]
            for sc in rng[2]:
                v = vb + dtype(sc) * h[2]
                v2 = (v * v).sum(-1)
                take = v2 < best                                         # (strict: ties keep the first)
                best = np.where(take, v2, best)
                out = np.where(take[..., None], v, out)
    return out


def image_terms(x, x0, x1, lam, cell, pbc, dtype=np.float64):
    """(S, F [n, 3]) of one image at positions ``x`` between the end points ``x0`` and ``x1``, in ``dtype``."""
    n = len(x)
    lam = dtype(lam)
    if n < 2:
        return dtype(0.0), np.zeros((n, 3), dtype=dtype)
    off = ~np.eye(n, dtype=bool)

    def pairs(y):
        y = np.asarray(y, dtype=dtype)
        D = nearest(y[None, :, :] - y[:, None, :], cell, pbc, dtype)     # D[i, j] = x_j - x_i
        return D, (D * D).sum(-1)
    D, d2 = pairs(x)
    d0, d1 = np.sqrt(pairs(x0)[1]), np.sqrt(pairs(x1)[1])
    d2 = np.where(off, d2, dtype(1.0))                                   # (the diagonal carries no term: w = 0 there)
    d = np.sqrt(d2)
    w = np.where(off, ((dtype(1.0) - lam) * d0 + lam * d1) - d, dtype(0.0))
    with np.errstate(divide="ignore", invalid="ignore"):
        i2 = dtype(1.0) / d2
        i4 = i2 * i2
        term = w * w * i4
        c = dtype(-2.0) * w * (d + dtype(2.0) * w) * i4 * i2             # c_ij / d_ij
        S = np.triu(term, 1).sum()
        F = (c[..., None] * D).sum(1)
    return S, F


def terms(positions, offsets, bands, cells, pbcs, dtype=np.float64):
    """(S [n_frames], F [N, 3]) of every image of every band (end points through the same formulas)."""
    x = np.asarray(positions, dtype=dtype).reshape(-1, 3)
    S = np.zeros(len(offsets) - 1, dtype=dtype)
    F = np.zeros_like(x)
    for b in range(len(bands) - 1):
        f0, M = bands[b], bands[b + 1] - bands[b]
        x0, x1 = x[offsets[f0]:offsets[f0 + 1]], x[offsets[f0 + M - 1]:offsets[f0 + M]]
        for k in range(M):
            f = f0 + k
            lam = dtype(k) / dtype(M - 1)
            S[f], F[offsets[f]:offsets[f + 1]] = image_terms(x[offsets[f]:offsets[f + 1]], x0, x1, lam, cells[f], pbcs[f], dtype)
    return S, F


def layout(bands):
    """(x0 [N, 3], offsets, band_first, cells, pbcs) of a list of bands of ``Atoms``."""
    frames = [a for b in bands for a in b]
    off = np.cumsum([0] + [len(a) for a in frames])
    first = np.cumsum([0] + [len(b) for b in bands])
    cells = [np.array(a.get_cell(), float).reshape(3, 3) for a in frames]
    pbcs = [np.asarray(a.get_pbc(), bool).reshape(3) for a in frames]
    return np.concatenate([a.get_positions() for a in frames]), off, first, cells, pbcs


def evaluate_bands(bands, positions=None, dtype=np.float64):
    x0, off, first, cells, pbcs = layout(bands)
    return terms(x0 if positions is None else positions, off, first, cells, pbcs, dtype)


def band_of(bands, spring=0.1, fixed=None):
    """The ``_neb_ref.Band`` of a list of bands whose energies are S and whose forces are F."""
    x0, off, first, cells, pbcs = layout(bands)

    def evaluate(x):
        S, F = terms(x, off, first, cells, pbcs)
        return np.asarray(S, float), np.asarray(F, float)
    return N.Band(evaluate, x0, off, first, spring=spring, fixed=fixed)


def min_distances(band):
    """The smallest nearest-image distance of every image of one band."""
    out = []
    for a in band:
        x = a.get_positions()
        D = nearest(x[None] - x[:, None], a.get_cell(), a.get_pbc())
        d = np.sqrt((D * D).sum(-1)) + 1e9 * np.eye(len(x))
        out.append(d.min())
    return np.array(out)


# ---- the bands of the tests ------------------------------------------------------------------------------------------------
def _rattled(atoms, seed, rattle):
    x = atoms.get_positions() + np.random.default_rng(seed).normal(0, rattle, (len(atoms), 3))
    return Atoms(numbers=atoms.get_atomic_numbers(), positions=x, cell=atoms.get_cell(), pbc=atoms.get_pbc())


def recelled(band, U=None, Q=None, pbc=None):
    """The band in the cell ``U @ cell`` (positions as they are: nearest images do not care where an atom is stored), turned by
    ``Q``, with ``pbc``."""
    out = []
    for a in band:
        cell, x = np.array(a.get_cell(), float).reshape(3, 3), a.get_positions()
        if U is not None:
            cell = np.asarray(U) @ cell
        if Q is not None:
            cell, x = cell @ np.asarray(Q).T, x @ np.asarray(Q).T
        out.append(Atoms(numbers=a.get_atomic_numbers(), positions=x, cell=cell, pbc=a.get_pbc() if pbc is None else pbc))
    return out


def _exchange(atoms, m, seed, rattle=(0.002, 0.005)):
    """tests/test_gpu_neb.py's ``_exchange`` (two neighbours of unlike species turning about their centre)."""
    import test_gpu_neb as T
    return T._exchange(atoms, m, seed, rattle)


def hop53(m=5, seed=3):
    """The vacancy hop in 3 x 3 x 3 bcc W (53 atoms), end points rattled, in the skewed re-description."""
    import test_gpu_neb as T
    return recelled(T._hop(m, seed, reps=(3, 3, 3)), U=SKEW)


def exchange16(m=6, seed=13):
    return _exchange(synthetic.lattice_frame("bcc", (2, 2, 2), 3.2, [42, 74], seed=21, rattle=0.0, strain=0.0), m, seed)


def exchange54_slab(m=4, seed=11):
    a = synthetic.lattice_frame("bcc", (3, 3, 3), 3.2, [42, 74], seed=84, rattle=0.0, strain=0.0)
    return recelled(_exchange(a, m, seed), pbc=[True, True, False])


def pair2(m=3):
    z = [74, 74]
    ini = Atoms(numbers=z, positions=[[0.0, 0.0, 0.0], [2.5, 0.1, -0.2]], cell=np.zeros((3, 3)), pbc=False)
    fin = Atoms(numbers=z, positions=[[0.1, 0.0, 0.05], [0.3, 2.2, 0.4]], cell=np.zeros((3, 3)), pbc=False)
    return neb.interpolate(ini, fin, m)


def single1(m=3):
    ini = Atoms(numbers=[74], positions=[[0.2, 0.3, 0.4]], cell=4.0 * np.eye(3), pbc=True)
    fin = Atoms(numbers=[74], positions=[[1.2, 0.1, 0.9]], cell=4.0 * np.eye(3), pbc=True)
    return neb.interpolate(ini, fin, m)


def cubic257(m=4, seed=17):
    """257 atoms in a cubic cell (a second chunk of one atom; rounding alone, no search): 4 x 4 x 4 fcc and an interstitial that
    moves from one octahedral site to the next, end points rattled independently."""
    a = synthetic.lattice_frame("fcc", (4, 4, 4), 4.0, [29], seed=0, rattle=0.0, strain=0.0)
    x = np.concatenate([a.get_positions(), [[2.0, 0.0, 0.0]]])
    y = x.copy()
    y[-1] = [0.0, 2.0, 0.0]
    z = np.full(len(x), 29)
    ini = Atoms(numbers=z, positions=x, cell=a.get_cell(), pbc=True)
    fin = Atoms(numbers=z, positions=y, cell=a.get_cell(), pbc=True)
    return neb.interpolate(_rattled(ini, seed, 0.002), _rattled(fin, seed + 1000, 0.02), m)


def batch():
    """The bands of the one-evaluation comparison, in the issue's order."""
    return [pair2(), single1(), cubic257(), hop53(), exchange54_slab(), exchange16()]


PARITY = {"hop53": (hop53, 0.1), "exchange16": (exchange16, 0.2), "cubic257": (cubic257, 0.3)}   # band, its spring


def straight_exchange_ends(seed=5):
    """The end points of the straight-line exchange of two neighbours in 3 x 3 x 3 bcc W (54 atoms) in the skewed cell: its
    linear band drives the two atoms through each other."""
    a = synthetic.lattice_frame("bcc", (3, 3, 3), A0_W, [74], seed=0, rattle=0.0, strain=0.0)
    x = a.get_positions()
    d = np.linalg.norm(x - x[0], axis=1)
    j = int(np.argsort(d)[1])
    ini = _rattled(a, seed, 0.002)
    y = _rattled(a, seed + 1000, 0.002).get_positions()
    y[[0, j]] = y[[j, 0]]
    fin = Atoms(numbers=a.get_atomic_numbers(), positions=y, cell=a.get_cell(), pbc=True)
    return recelled([ini], U=SKEW)[0], recelled([fin], U=SKEW)[0]


@functools.lru_cache(None)
def parity_run(name, n_first=30, n_more=400, fmax=1e-2):
    """The restatement's run of a parity band: what the device is compared with, and the conditions on it."""
    make, spring = PARITY[name]
    ref = band_of([make()], spring=spring)
    kw = dict(dt=0.1, dt_max=1.0, maxstep=0.2)
    first = []
    for _ in range(n_first):
        ref.run(1, fmax=fmax, **kw)
        first.append((ref.x.copy(), ref.e_last.copy(), ref.crit.copy(), ref.status.copy()))
    ref.run(n_more, fmax=fmax, **kw)
    return dict(first=first, x=ref.x.copy(), status=ref.status.copy(), steps=ref.steps.copy(), margins=np.array(ref.margins),
                crit=ref.crit.copy(), spring=spring)
