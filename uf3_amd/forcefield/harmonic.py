"""
Harmonic properties from the exact second derivatives of the UF3 energy (``uf3_hessian``).

The device computes, for one frame, the Hessian of the energy the evaluator computes (periodic images folded onto their
parent atom: the Gamma-point force constants of the frame), its mixed position / strain derivatives and the clamped-ion strain
term.  On top of those, this module builds what the reference obtains from ``phonopy``, ``seekpath`` and ``elastic`` by finite
differences (``calculator.py:449-487``, ``properties/phonon.py``, ``properties/elastic.py``): phonon frequencies and bands on
a diagonal supercell, and the relaxed-ion elastic tensor.  There is no displacement or strain step.

Units: Angstrom, eV, amu; frequencies in THz (imaginary modes as negative numbers, as phonopy reports them); stresses and
elastic constants in GPa.
"""
import ctypes as C
import itertools
import warnings

import numpy as np

from .. import _lib
from ..data.atoms import Atoms
from .md import resolve_masses

EV_PER_A3_GPA = 160.21766208           # 1 eV / Angstrom^3 in GPa
THZ = 15.633302                        # sqrt(eV / (amu Angstrom^2)) / (2 pi), in THz

_VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def _frame(atoms):
    n = len(atoms.get_atomic_numbers())
    if n < 1:
        raise ValueError("harmonic: the frame has no atoms")
    return n


def _periodic(atoms, what):
    if not np.all(np.asarray(atoms.get_pbc(), dtype=bool)):
        raise ValueError(f"harmonic.{what}: needs a frame periodic along all three axes")


def _row_span(rows, n):
    if rows is None:
        return 0, n
    if isinstance(rows, range):
        if rows.step != 1:
            raise ValueError("harmonic.hessian: rows must be contiguous")
        lo, hi = rows.start, rows.stop
    elif isinstance(rows, slice):
        if rows.step not in (None, 1):
            raise ValueError("harmonic.hessian: rows must be contiguous")
        lo, hi, _ = rows.indices(n)
    else:
        lo, hi = (int(v) for v in rows)
    if not (0 <= lo < hi <= n):
        raise ValueError(f"harmonic.hessian: row span [{lo}, {hi}) empty or outside the frame's {n} atoms")
    return int(lo), int(hi)


def hessian(calc, atoms, rows=None, strain=False):
    """
    d2E / dx dx' of one frame on the device: H [3N, 3N], or the rows of atoms ``rows`` (a ``range``, a ``slice`` or a pair
    ``(begin, end)``) as [3R, 3N].  With ``strain=True`` (whole frame only): ``(H, mixed [3N, 6], born [6, 6], virial [6])``,
    mixed = d2E / dx dt_v = -dF / dt_v and born = d2E / dt_u dt_v at fixed fractional coordinates, t the strain of the
    evaluator's virial (Voigt xx, yy, zz, yz, xz, xy; eV).  Non-periodic axes are allowed.
    """
    n = _frame(atoms)
    lo, hi = _row_span(rows, n)
    if strain and (lo, hi) != (0, n):
        raise ValueError("harmonic.hessian: strain=True needs the whole frame's rows")
    ctx = _lib.get_context(calc.device)
    db = _lib.device_basis(calc.bspline_config, ctx)
    batch = _lib.FrameBatch([atoms])
    H = np.empty((3 * (hi - lo), 3 * n))
    mixed = np.empty((3 * n, 6)) if strain else None
    born = np.empty((6, 6)) if strain else None
    addr = _lib._addr
    rc = ctx.lib.uf3_hessian(db.handle, C.byref(batch.struct), addr(batch.pos), addr(batch.z), calc._pc[0], calc._pc[1],
                             calc._pc[2], lo, hi, addr(H), addr(mixed), addr(born))
    ctx.check(rc)
    if not strain:
        return H
    _, _, _, v = calc.evaluate_frames([atoms], forces=True, virial=True)
    return H, mixed, born, np.asarray(v[0], dtype=float)


def force_constants(calc, atoms):
    """Force constants [N, N, 3, 3] (phonopy's layout) of the frame: the Hessian with periodic images folded."""
    n = _frame(atoms)
    return hessian(calc, atoms).reshape(n, 3, n, 3).transpose(0, 2, 1, 3).copy()


# ------------------------------------------------------------------------------------------------------------- phonons
def supercell(atoms, n_super):
    """The n_super^3 diagonal supercell: atom ``(a * n + b) * n + c) * N + i`` is atom i shifted by (a, b, c) cells."""
    n_super = int(n_super)
    if n_super < 1:
        raise ValueError("harmonic: n_super must be >= 1")
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    pos = np.asarray(atoms.get_positions(), dtype=float).reshape(-1, 3)
    shifts = np.array(list(itertools.product(range(n_super), repeat=3)), dtype=float)
    sc_pos = (shifts @ cell)[:, None, :] + pos[None, :, :]
    numbers = np.tile(np.asarray(atoms.get_atomic_numbers()), len(shifts))
    return Atoms(numbers=numbers, positions=sc_pos.reshape(-1, 3), cell=cell * n_super, pbc=True)


def minimum_image_weights(cell, pos, n_super, tol=1e-5):
    """For every primitive atom i and supercell atom p = (image, j): the lattice vectors R (Cartesian, [3]) of the equivalent
    images of p nearest to atom i, each with weight 1 / multiplicity (phonopy's convention).  Returns a list over (i, p) of
    (R [k, 3], weight) -- R is the primitive-lattice vector from the cell of i to the chosen image of p's cell."""
    cell = np.asarray(cell, dtype=float).reshape(3, 3)
    pos = np.asarray(pos, dtype=float).reshape(-1, 3)
    n = len(pos)
    shifts = np.array(list(itertools.product(range(n_super), repeat=3)), dtype=float)
    sup = cell * n_super
    around = np.array(list(itertools.product((-2, -1, 0, 1, 2), repeat=3)), dtype=float) @ sup
    out = []
    for i in range(n):
        row = []
        for t in shifts:
            base = t @ cell
            for j in range(n):
                v = base + pos[j] - pos[i] + around
                d = np.linalg.norm(v, axis=1)
                near = d <= d.min() + tol
                row.append((base + around[near], 1.0 / int(near.sum())))
        out.append(row)
    return out


def _masses(atoms, masses):
    """``md.resolve_masses`` for one frame: a dict {symbol or Z: amu}, a per-atom array, or ``atoms.get_masses()`` (ASE
    frames; the package's own ``Atoms`` has none, so pass ``masses`` with those)."""
    try:
        return resolve_masses([atoms], masses)
    except ValueError as e:
        raise ValueError(str(e).replace("MolecularDynamics:", "harmonic:")) from None


def dynamical_matrices(fc_rows, atoms, qpoints, n_super, masses):
    """D(q) [nq, 3N, 3N] from the rows of the supercell force constants fc_rows [N, N_sc, 3, 3] (primitive atoms in image
    (0, 0, 0)), q in reduced coordinates of the cell's reciprocal lattice, minimum-image weights."""
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    pos = np.asarray(atoms.get_positions(), dtype=float).reshape(-1, 3)
    n = len(pos)
    q = np.atleast_2d(np.asarray(qpoints, dtype=float))
    kc = q @ np.linalg.inv(cell).T                 # Cartesian wave vectors without 2 pi: exp(2 pi i k . R)
    w = minimum_image_weights(cell, pos, n_super)
    inv_sqrt_m = 1.0 / np.sqrt(np.asarray(masses, dtype=float))
    D = np.zeros((len(q), 3 * n, 3 * n), dtype=complex)
    n_img = n_super ** 3
    for i in range(n):
        for p in range(n_img * n):
            j = p % n
            R, wt = w[i][p]
            phase = wt * np.exp(2j * np.pi * (kc @ R.T)).sum(axis=1)
            D[:, 3 * i:3 * i + 3, 3 * j:3 * j + 3] += phase[:, None, None] * fc_rows[i, p][None]
    scale = np.repeat(inv_sqrt_m, 3)
    D *= scale[None, :, None] * scale[None, None, :]
    return 0.5 * (D + np.conj(np.transpose(D, (0, 2, 1))))


def frequencies_from(D, eigenvectors=False):
    """THz from dynamical matrices [nq, 3N, 3N] (eV / (amu A^2)); negative numbers for imaginary modes."""
    if eigenvectors:
        lam, vec = np.linalg.eigh(D)
    else:
        lam, vec = np.linalg.eigvalsh(D), None
    f = np.sign(lam) * np.sqrt(np.abs(lam)) * THZ
    return (f, vec) if eigenvectors else f


def _supercell_rows(calc, atoms, n_super):
    n = _frame(atoms)
    sc = supercell(atoms, n_super)
    rows = hessian(calc, sc, rows=(0, n))
    return rows.reshape(n, 3, -1, 3).transpose(0, 2, 1, 3)


def phonon_frequencies(calc, atoms, qpoints, n_super=5, masses=None, eigenvectors=False):
    """Phonon frequencies [nq, 3N] (THz) at reduced wave vectors ``qpoints`` [nq, 3] of the cell's reciprocal lattice, from
    the device Hessian of the n_super^3 diagonal supercell (what the reference passes to phonopy) with phonopy's
    minimum-image convention.  Masses: ``md.resolve_masses`` rules.  ``eigenvectors=True`` also returns [nq, 3N, 3N]."""
    _periodic(atoms, "phonon_frequencies")
    m = _masses(atoms, masses)
    fc = _supercell_rows(calc, atoms, n_super)
    return frequencies_from(dynamical_matrices(fc, atoms, qpoints, n_super, m), eigenvectors)


# path recognition: the three cubic Bravais lattices with axes along x, y, z, seekpath's labels
_PATHS = {
    "cP": ({"GAMMA": (0, 0, 0), "X": (0, 0.5, 0), "M": (0.5, 0.5, 0), "R": (0.5, 0.5, 0.5)},
           [("GAMMA", "X"), ("X", "M"), ("M", "GAMMA"), ("GAMMA", "R"), ("R", "X"), ("R", "M")]),
    "cI": ({"GAMMA": (0, 0, 0), "H": (0, 0, 1), "N": (0.5, 0.5, 0), "P": (0.5, 0.5, 0.5)},
           [("GAMMA", "H"), ("H", "N"), ("N", "GAMMA"), ("GAMMA", "P"), ("P", "H"), ("P", "N")]),
    "cF": ({"GAMMA": (0, 0, 0), "X": (0, 1, 0), "U": (0.25, 1, 0.25), "K": (0.75, 0.75, 0), "L": (0.5, 0.5, 0.5),
            "W": (0.5, 1, 0)},
           [("GAMMA", "X"), ("X", "U"), ("K", "GAMMA"), ("GAMMA", "L"), ("L", "W"), ("W", "X")]),
}
_CENTRING = {"cP": [], "cI": [(0.5, 0.5, 0.5)], "cF": [(0, 0.5, 0.5), (0.5, 0, 0.5), (0.5, 0.5, 0)]}
_POINTS_PER_CELL = {"cP": 1, "cI": 2, "cF": 4}


def _translations(atoms, tol=1e-5):
    """Pure translations (fractional, inside the cell) that map the structure onto itself, the zero vector first."""
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    frac = np.asarray(atoms.get_positions(), dtype=float).reshape(-1, 3) @ np.linalg.inv(cell)
    z = np.asarray(atoms.get_atomic_numbers())
    out = []
    for j in np.flatnonzero(z == z[0]):
        t = frac[j] - frac[0]
        t -= np.floor(t + tol)
        moved = frac + t
        ok = True
        for i in range(len(frac)):
            d = moved[i] - frac
            d -= np.round(d)
            hit = np.flatnonzero(np.all(np.abs(d @ cell) < tol * 10, axis=1))
            if len(hit) == 0 or z[hit[0]] != z[i]:
                ok = False
                break
        if ok:
            out.append(t)
    return np.array(out)


def cubic_lattice(atoms, tol=1e-6):
    """('cP' | 'cI' | 'cF', a) when the crystal's lattice (cell + pure translations of the structure) is simple, body- or
    face-centred cubic with its cube axes along x, y, z; None otherwise."""
    if not np.all(np.asarray(atoms.get_pbc(), dtype=bool)):
        return None
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    vol = abs(np.linalg.det(cell))
    if vol <= 0:
        return None
    inv = np.linalg.inv(cell)
    tr = _translations(atoms)
    per_point = vol / len(tr)
    for kind in ("cF", "cI", "cP"):
        a = (_POINTS_PER_CELL[kind] * per_point) ** (1.0 / 3.0)
        gens = [np.eye(3)[k] for k in range(3)] + [np.array(c, dtype=float) for c in _CENTRING[kind]]
        ok = True
        for g in gens:
            f = (a * g) @ inv
            d = f[None, :] - tr
            d -= np.round(d)
            if not np.any(np.all(np.abs(d @ cell) < tol * max(1.0, a), axis=1)):
                ok = False
                break
        if ok:
            return kind, a
    return None


def standard_path(atoms):
    """seekpath's labels and path for a cubic crystal (``cubic_lattice``): (point_coords {label: reduced q of the given
    cell}, path [(label, label)]).  ValueError for any other cell."""
    found = cubic_lattice(atoms)
    if found is None:
        raise ValueError("harmonic: the cell is not recognised as a simple, body- or face-centred cubic lattice with its axes "
                         "along x, y, z: pass an explicit path, a list of segments ((label, reduced q), (label, reduced q))")
    kind, a = found
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    pts, path = _PATHS[kind]
    coords = {k: (cell @ (np.asarray(v, dtype=float) / a)).round(12) + 0.0 for k, v in pts.items()}
    return {k: [float(x) for x in v] for k, v in coords.items()}, list(path)


def band_structure(calc, atoms, path=None, n_super=5, resolution=30, masses=None):
    """
    Phonon bands along a path, in the reference's shapes (``properties/phonon.py``): ``(force_constants, path_data,
    bands_dict)``.  force_constants [N, N * n_super^3, 3, 3]: the rows of the primitive atoms (phonopy's compact layout).
    path_data: ``point_coords`` {label: reduced q} and ``path`` [(label, label)].  bands_dict: ``qpoints``, ``distances``,
    ``frequencies`` (THz), ``eigenvectors``, one entry per segment with ``resolution + 1`` points each.  ``path=None``:
    seekpath's path of a cubic crystal (``standard_path``); otherwise a list of segments ((label, q), (label, q)).
    """
    _periodic(atoms, "band_structure")
    m = _masses(atoms, masses)
    resolution = int(resolution)
    if resolution < 1:
        raise ValueError("harmonic.band_structure: resolution must be >= 1")
    if path is None:
        coords, segs = standard_path(atoms)
    else:
        coords, segs = {}, []
        for seg in path:
            (la, qa), (lb, qb) = seg
            coords[str(la)] = [float(x) for x in qa]
            coords[str(lb)] = [float(x) for x in qb]
            segs.append((str(la), str(lb)))
    fc = _supercell_rows(calc, atoms, n_super)
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    recip = np.linalg.inv(cell).T                  # rows: reciprocal vectors without 2 pi
    qs, dists, freqs, vecs = [], [], [], []
    start = 0.0
    for la, lb in segs:
        qa, qb = np.asarray(coords[la]), np.asarray(coords[lb])
        q = np.array([qa + (qb - qa) * k / resolution for k in range(resolution + 1)])
        step = np.linalg.norm((qb - qa) @ recip) / resolution
        d = start + step * np.arange(resolution + 1)
        start = d[-1]
        f, v = frequencies_from(dynamical_matrices(fc, atoms, q, n_super, m), eigenvectors=True)
        qs.append(q); dists.append(d); freqs.append(f); vecs.append(v)
    path_data = {"point_coords": coords, "path": segs}
    bands = {"qpoints": qs, "distances": dists, "frequencies": freqs, "eigenvectors": vecs}
    return fc, path_data, bands


# ----------------------------------------------------------------------------------------------------- elastic constants
def relaxed_tensor(H, mixed, born):
    """B - mixed^T H^+ mixed (eV), H^+ the pseudo-inverse of H with the three rigid translations projected out: the
    second strain derivative of the energy minimised over the internal coordinates (the ions' relaxation)."""
    H = np.asarray(H, dtype=float)
    n3 = H.shape[0]
    T = np.zeros((n3, 3))
    for k in range(3):
        T[k::3, k] = 1.0
    T /= np.linalg.norm(T, axis=0)
    P = np.eye(n3) - T @ T.T
    Hp = P @ (0.5 * (H + H.T)) @ P
    w, V = np.linalg.eigh(Hp)
    cut = max(np.abs(w).max(), 1e-300) * 1e-10
    inv = np.where(np.abs(w) > cut, 1.0 / np.where(np.abs(w) > cut, w, 1.0), 0.0)
    Lp = P @ np.asarray(mixed, dtype=float)
    return np.asarray(born, dtype=float) - (Lp.T @ V) @ (inv[:, None] * (V.T @ Lp))


def elastic_tensor(calc, atoms, relaxed=True):
    """
    Elastic constants from the exact second derivatives: dict(C [6, 6] GPa -- relaxed ions, (B - mixed^T H^+ mixed) / V, or
    clamped with ``relaxed=False`` --, C_clamped = B / V, bulk_modulus (Voigt, GPa), stress [6] GPa).  Voigt order xx, yy, zz,
    yz, xz, xy, engineering shear strains.  Fully periodic frames only.  Warns when |stress| > 1e-3 max|C|: the second
    derivative is then not the stress-strain slope.
    """
    _periodic(atoms, "elastic_tensor")
    H, mixed, born, vir = hessian(calc, atoms, strain=True)
    vol = abs(float(np.linalg.det(np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3))))
    clamped = born / vol * EV_PER_A3_GPA
    C = relaxed_tensor(H, mixed, born) / vol * EV_PER_A3_GPA if relaxed else clamped
    C = 0.5 * (C + C.T)
    stress = vir / vol * EV_PER_A3_GPA
    if np.abs(stress).max() > 1e-3 * np.abs(C).max():
        warnings.warn(f"harmonic.elastic_tensor: the frame is under stress (max |stress| {np.abs(stress).max():.3g} GPa): "
                      "the second derivative is not the stress-strain slope", RuntimeWarning)
    bulk = (C[0, 0] + C[1, 1] + C[2, 2] + 2.0 * (C[0, 1] + C[0, 2] + C[1, 2])) / 9.0
    return {"C": C, "C_clamped": 0.5 * (clamped + clamped.T), "bulk_modulus": float(bulk), "stress": stress}


def cubic_constants(C, tol=1e-6):
    """[C11, C12, C44, B] (B = (C11 + 2 C12) / 3) when C [6, 6] has cubic form within tol * max|C|; ValueError otherwise."""
    C = np.asarray(C, dtype=float)
    scale = np.abs(C).max() * tol
    c11, c12, c44 = np.mean(np.diag(C)[:3]), np.mean([C[0, 1], C[0, 2], C[1, 2]]), np.mean(np.diag(C)[3:])
    ref = np.zeros((6, 6))
    ref[:3, :3] = c12
    ref[[0, 1, 2], [0, 1, 2]] = c11
    ref[[3, 4, 5], [3, 4, 5]] = c44
    if np.abs(C - ref).max() > scale:
        raise ValueError("harmonic: the elastic tensor does not have cubic form in the cell's frame; "
                         "use harmonic.elastic_tensor for the full tensor")
    return [float(c11), float(c12), float(c44), float((c11 + 2.0 * c12) / 3.0)]
