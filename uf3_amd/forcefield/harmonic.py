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
PLANCK_EV_PER_THZ = 4.135667696e-3     # h in eV / THz (CODATA 2018)
KB_EV_PER_K = 8.617333262e-5           # k_B in eV / K (CODATA 2018)
MESH_MAX_ATOMS = 32                    # uf3_phonon_mesh: D(q) of a wave lives in LDS, 16 (3N)^2 bytes

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


def _pair_reduced(sup):
    """``(red, M)``: a basis ``red = M @ sup`` of the lattice of ``sup``'s rows, M integer with det +-1, in which no row gets
    shorter by adding a multiple of another (Gauss's reduction, pair by pair until nothing changes).  It only keeps the search
    of ``nearest_images`` small on a skewed description; any basis of the lattice gives the same images."""
    red = np.array(sup, dtype=float)
    M = np.eye(3, dtype=np.int64)
    changed = True
    while changed:
        changed = False
        for a in range(3):
            for b in range(3):
                k = int(np.rint((red[a] @ red[b]) / (red[b] @ red[b]))) if a != b else 0
                if k:
                    new = red[a] - k * red[b]
                    if new @ new < (red[a] @ red[a]) * (1.0 - 1e-12):
                        red[a], changed = new, True
                        M[a] -= k * M[b]
    return M.astype(float) @ np.asarray(sup, dtype=float), M


_IMAGE_CHUNK = 1 << 22                 # candidate translations held at a time by nearest_images


def nearest_images(sup, v, tol=1e-5):
    """The translations of the lattice of ``sup``'s rows that bring the separations ``v`` [P, 3] nearest to the origin:
    ``(pair int64 [m], K int64 [m, 3], mult int64 [P], examined int64 [P])`` -- for every pair, in order, each integer triple K
    with ``|v + K @ sup| <= min + tol``, in the order of the triple; ``mult`` their number and ``examined`` the number of
    candidate translations the pair's search box holds.

    Every such translation is found, for any basis of the lattice and any ``v`` (atoms outside their cell included); the search
    is sized from the geometry.  With ``red = M @ sup`` the pair-reduced basis, ``v`` is taken into red's fractional
    [-1/2, 1/2)^3, which gives a lattice image of length L; an image no longer than L + tol has |fractional coordinate a| <=
    (L + tol) / h_a, h_a the spacing of red's lattice planes a, and those integer boxes are the candidates: 8 to 27 per pair
    on a compact cell.  The lengths are those of ``(v + K @ sup)`` evaluated in that order."""
    sup = np.asarray(sup, dtype=float).reshape(3, 3)
    v = np.asarray(v, dtype=float).reshape(-1, 3)
    red, M = _pair_reduced(sup)
    inv = np.linalg.inv(red)
    per_h = np.sqrt((inv * inv).sum(axis=0))                     # 1 / h_a: |column a of red^-1|
    f = v @ inv
    if not np.all(np.abs(f) < 2.0 ** 52):
        raise ValueError("harmonic.nearest_images: a separation is not finite, or too many cells long to resolve a lattice vector")
    n0 = -np.floor(f + 0.5)
    fr = f + n0
    reach = (np.sqrt((((fr @ red)) ** 2).sum(axis=1)) + tol)[:, None] * per_h[None, :] * (1.0 + 1e-9) + 1e-12
    lo = np.ceil(-reach - fr).astype(np.int64)
    hi = np.floor(reach - fr).astype(np.int64)
    assert np.all(hi >= lo)
    n0 = n0.astype(np.int64)
    examined = (hi - lo + 1).prod(axis=1)
    pairs, Ks, mult = [], [], np.empty(len(v), dtype=np.int64)
    start = 0
    while start < len(v):
        # as many pairs at a time as keep the padded box of candidates within _IMAGE_CHUNK
        stop, width = start, np.zeros(3, dtype=np.int64)
        if (len(v) - start) * int((hi - lo + 1)[start:].max(axis=0).prod()) <= _IMAGE_CHUNK:
            stop, width = len(v), (hi - lo + 1)[start:].max(axis=0)
        while stop < len(v):
            wider = np.maximum(width, hi[stop] - lo[stop] + 1)
            if stop > start and (stop + 1 - start) * int(wider.prod()) > _IMAGE_CHUNK:
                break
            width, stop = wider, stop + 1
        off = np.array(list(itertools.product(*(range(int(x)) for x in width))), dtype=np.int64)      # [W, 3], triple order
        valid = np.all(off[None, :, :] <= (hi - lo)[start:stop, None, :], axis=-1)
        K = ((n0 + lo)[start:stop, None, :] + off[None, :, :]) @ M                                 # triples of sup's own rows
        w = v[start:stop, None, :] + (K.reshape(-1, 3).astype(float) @ sup).reshape(K.shape)
        d = np.where(valid, np.sqrt((w * w).sum(axis=-1)), np.inf)
        near = d <= d.min(axis=-1, keepdims=True) + tol
        p_idx, c_idx = np.nonzero(near)
        mult[start:stop] = near.sum(axis=-1)
        pairs.append(p_idx + start)
        Ks.append(K[p_idx, c_idx])
        start = stop
    pair, K = np.concatenate(pairs), np.concatenate(Ks)
    order = np.lexsort((K[:, 2], K[:, 1], K[:, 0], pair))
    return pair[order], K[order], mult, examined


def _cell_images(cell, pos, n_super, tol):
    """``nearest_images`` for every primitive atom i against the atoms of the n_super^3 supercell: a generator of
    ``(i, p int64 [m], K int64 [m, 3], n int64 [m, 3], mult int64 [m])``, the records of atom i in the order p, then triple; K
    the supercell translation and n = shift + n_super K the triple of the image's lattice vector R = n @ cell.  The separations
    are ((shift @ cell + pos_j) - pos_i), in that order."""
    shifts_i = np.array(list(itertools.product(range(n_super), repeat=3)), dtype=np.int64)
    base = shifts_i.astype(float) @ cell
    sup = cell * n_super
    n = len(pos)
    for i in range(n):
        v = ((base[:, None, :] + pos[None, :, :]) - pos[i]).reshape(-1, 3)
        p, K, mult, _ = nearest_images(sup, v, tol)
        yield i, p, K, shifts_i[p // n] + n_super * K, mult[p]


def minimum_image_weights(cell, pos, n_super, tol=1e-5):
    """For every primitive atom i and supercell atom p = (image, j): the lattice vectors R (Cartesian, [3]) of the equivalent
    images of p nearest to atom i, each with weight 1 / multiplicity (phonopy's convention).  Returns a list over (i, p) of
    (R [k, 3], weight) -- R is the primitive-lattice vector from the cell of i to the chosen image of p's cell.  All the images
    within ``tol`` of the nearest one are found (``nearest_images``), however the cell is described -- skewed, turned, or with
    atoms outside it."""
    cell = np.asarray(cell, dtype=float).reshape(3, 3)
    pos = np.asarray(pos, dtype=float).reshape(-1, 3)
    n_super = int(n_super)
    shifts = np.array(list(itertools.product(range(n_super), repeat=3)), dtype=float)
    sup = cell * n_super
    out = []
    for _, p, K, _, _ in _cell_images(cell, pos, n_super, tol):
        R = (shifts[p // len(pos)] @ cell) + K.astype(float) @ sup
        cuts = np.flatnonzero(np.diff(p)) + 1
        out.append([(r, 1.0 / len(r)) for r in np.split(R, cuts)])
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


# ------------------------------------------------------------------------------------------- phonons on a q-mesh (device)
# DESIGN.md section 3.12.  D(q) and its eigenvalues at every q-point of a mesh, the density of states and the harmonic
# thermodynamics run on the device (uf3_phonon_mesh / _dos / _thermo); the force constants come from one uf3_hessian call per
# structure.  Eigenvectors on the mesh (projected DOS, thermal displacements, group velocities): further down.  Out of scope:
# the tetrahedron method, point-group reduction of the mesh, non-analytic (LO-TO) corrections, the quasi-harmonic volume loop,
# plotting.
def qmesh(mesh, gamma_centred=True, time_reversal=True):
    """Regular mesh of reduced wave vectors: ``(q [nq, 3] in [0, 1), weights int64 [nq])``.  q_k = a_k / n_k, a_k = 0 .. n_k - 1,
    or (a_k + 1/2) / n_k with ``gamma_centred=False``.  With ``time_reversal`` one of each pair (q, -q mod 1) is kept with
    weight 2 (the first in mesh order), self-conjugate points with weight 1; the weights always sum to n_1 n_2 n_3.  There is
    no point-group reduction."""
    mesh = np.asarray(mesh, dtype=np.int64).reshape(-1)
    if mesh.shape != (3,) or np.any(mesh < 1):
        raise ValueError("harmonic.qmesh: mesh must be three positive integers")
    a = np.stack(np.meshgrid(*(np.arange(n) for n in mesh), indexing="ij"), axis=-1).reshape(-1, 3)
    weights = np.ones(len(a), dtype=np.int64)
    if time_reversal:
        partner = (-a) % mesh if gamma_centred else mesh - 1 - a
        own = np.ravel_multi_index(tuple(a.T), tuple(mesh))
        other = np.ravel_multi_index(tuple(partner.T), tuple(mesh))
        keep = own <= other
        weights = np.where(own == other, 1, 2).astype(np.int64)[keep]
        a = a[keep]
    q = (a + (0.0 if gamma_centred else 0.5)) / mesh
    return np.ascontiguousarray(q), np.ascontiguousarray(weights)


def image_terms(atoms, n_super, tol=1e-5):
    """``minimum_image_weights`` as a flat list for the device: ``(terms int32 [n_terms, 5], weights [n_terms])``, one record
    (i, p, n0, n1, n2) per chosen image -- primitive atom i, supercell atom p, and the lattice vector R = n @ cell of that
    image as integers, an integer combination of the cell's rows -- in the order of that function: i, then p, then the images
    in the order of the triple.  Any valid description of the cell is accepted (``nearest_images``); a triple that does not fit
    an int32 raises ValueError."""
    n_super = int(n_super)
    if n_super < 1:
        raise ValueError("harmonic: n_super must be >= 1")
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    pos = np.asarray(atoms.get_positions(), dtype=float).reshape(-1, 3)
    terms, weights = [], []
    for i, p, _, nvec, mult in _cell_images(cell, pos, n_super, tol):
        if np.abs(nvec).max() > np.iinfo(np.int32).max:
            raise ValueError("harmonic.image_terms: a lattice vector's integer components do not fit 32 bits; wrap the atoms "
                             "into the cell")
        rec = np.empty((len(p), 5), dtype=np.int32)
        rec[:, 0] = i
        rec[:, 1] = p
        rec[:, 2:] = nvec
        terms.append(rec)
        weights.append(1.0 / mult)
    return np.ascontiguousarray(np.concatenate(terms)), np.ascontiguousarray(np.concatenate(weights))


def eigenvalues_to_frequencies(lam):
    """THz from eigenvalues of D (eV / (amu A^2)); negative numbers for imaginary modes (``frequencies_from``'s rule)."""
    lam = np.asarray(lam, dtype=float)
    return np.sign(lam) * np.sqrt(np.abs(lam)) * THZ


def _mesh_context(device=None):
    return _lib.get_context(device)


def mesh_eigenvalues(fc_rows, atoms, qpoints, n_super, masses, device=None):
    """Eigenvalues of D(q) on the device (``uf3_phonon_mesh``): ``(lam [nq, 3N] ascending, eV / (amu A^2); sweeps int32 [nq])``.
    fc_rows [N, N_sc, 3, 3] and per-atom masses as for ``dynamical_matrices``, whose D(q) this diagonalises (the same sum in
    another order: agreement to rounding).  Cells of more than ``MESH_MAX_ATOMS`` atoms raise ValueError -- there is no host
    fallback; a q-point whose Jacobi iteration hits its sweep cap raises RuntimeError."""
    n = _frame(atoms)
    if n > MESH_MAX_ATOMS:
        raise ValueError(f"harmonic: the q-mesh eigensolver takes cells of at most {MESH_MAX_ATOMS} atoms (D(q) is held in LDS), "
                         f"this one has {n}")
    fc = np.asarray(fc_rows, dtype=float)
    n_sc = n * int(n_super) ** 3
    if fc.shape != (n, n_sc, 3, 3):
        raise ValueError(f"harmonic.mesh_eigenvalues: fc_rows must be [{n}, {n_sc}, 3, 3], got {fc.shape}")
    q = np.ascontiguousarray(np.atleast_2d(np.asarray(qpoints, dtype=float)))
    if q.ndim != 2 or q.shape[1] != 3 or len(q) < 1:
        raise ValueError("harmonic.mesh_eigenvalues: qpoints must be [nq, 3] with nq >= 1")
    m = np.asarray(masses, dtype=float).reshape(-1)
    if m.shape != (n,) or np.any(m <= 0):
        raise ValueError("harmonic.mesh_eigenvalues: one positive mass per atom")
    flat = np.ascontiguousarray(fc.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n_sc))
    inv_sqrt_m = np.ascontiguousarray(1.0 / np.sqrt(m))
    terms, w = image_terms(atoms, n_super)
    lam = np.empty((len(q), 3 * n))
    status = np.empty(len(q), dtype=np.int32)
    ctx = _mesh_context(device)
    addr = _lib._addr
    ctx.check(ctx.lib.uf3_phonon_mesh(ctx.handle, n, n_sc, addr(flat), addr(inv_sqrt_m), len(terms), addr(terms), addr(w), len(q),
                                      addr(q), addr(lam), addr(status)))
    if np.any(status < 0):
        bad = np.flatnonzero(status < 0)
        raise RuntimeError(f"harmonic.mesh_eigenvalues: the Jacobi iteration did not converge within its sweep cap at {len(bad)} "
                           f"q-point(s), the first q = {q[bad[0]].tolist()}")
    return lam, status


def _weights(weights, nq):
    if weights is None:
        return None
    w = np.ascontiguousarray(weights, dtype=np.int64).reshape(-1)
    if w.shape != (nq,) or np.any(w < 0):
        raise ValueError("harmonic: one non-negative integer weight per q-point")
    return w


def dos_from_eigenvalues(lam, weights=None, edges=None, samples=None, sigma=None, device=None):
    """``uf3_phonon_dos`` on eigenvalues lam [nq, n_modes]: ``(counts int64 [len(edges) - 1] or None, dos [len(samples)] or
    None)``.  counts: numpy's histogram rule over ``edges`` (THz), weighted by the integer q-weights.  dos: Gaussians of width
    ``sigma`` (THz) at ``samples``, normalised per q-point (its integral is the number of modes per cell)."""
    lam = np.ascontiguousarray(lam, dtype=float)
    if lam.ndim != 2 or lam.size == 0:
        raise ValueError("harmonic.dos_from_eigenvalues: lam must be [nq, n_modes]")
    nq, nm = lam.shape
    w = _weights(weights, nq)
    counts = dos = None
    if edges is not None:
        edges = np.ascontiguousarray(edges, dtype=float).reshape(-1)
        if len(edges) < 2 or np.any(np.diff(edges) <= 0):
            raise ValueError("harmonic.dos_from_eigenvalues: edges must be strictly increasing")
        counts = np.zeros(len(edges) - 1, dtype=np.int64)
    if samples is not None:
        samples = np.ascontiguousarray(samples, dtype=float).reshape(-1)
        if sigma is None or not float(sigma) > 0:
            raise ValueError("harmonic.dos_from_eigenvalues: sigma must be positive")
        dos = np.zeros(len(samples))
    if counts is None and dos is None:
        raise ValueError("harmonic.dos_from_eigenvalues: give edges, samples or both")
    ctx = _mesh_context(device)
    addr = _lib._addr
    ctx.check(ctx.lib.uf3_phonon_dos(ctx.handle, nm, nq, addr(lam), addr(w), 0 if counts is None else len(counts), addr(edges),
                                     addr(counts), 0 if dos is None else len(dos), addr(samples),
                                     float(sigma) if dos is not None else 0.0, addr(dos)))
    return counts, dos


def thermo_from_eigenvalues(lam, temperatures, weights=None, cutoff_THz=1e-3, device=None):
    """``uf3_phonon_thermo`` on eigenvalues lam [nq, n_modes]: dict of ``temperatures`` (K), ``free_energy``, ``internal_energy``
    (eV per cell), ``entropy``, ``heat_capacity`` (eV / K per cell), each [nT]; ``zero_point_energy`` (eV) and ``n_excluded``, the
    summed q-weight of the modes with f <= cutoff_THz, which are left out of every sum."""
    lam = np.ascontiguousarray(lam, dtype=float)
    if lam.ndim != 2 or lam.size == 0:
        raise ValueError("harmonic.thermo_from_eigenvalues: lam must be [nq, n_modes]")
    nq, nm = lam.shape
    w = _weights(weights, nq)
    T = np.ascontiguousarray(np.atleast_1d(np.asarray(temperatures, dtype=float)).reshape(-1))
    if len(T) < 1 or not np.all(np.isfinite(T)) or np.any(T < 0):
        raise ValueError("harmonic.thermo_from_eigenvalues: temperatures must be finite and >= 0")
    if not float(cutoff_THz) >= 0:
        raise ValueError("harmonic.thermo_from_eigenvalues: cutoff_THz must be >= 0")
    out = np.empty((len(T), 4))
    zpe = np.empty(1)
    n_excl = np.empty(1, dtype=np.int64)
    ctx = _mesh_context(device)
    addr = _lib._addr
    ctx.check(ctx.lib.uf3_phonon_thermo(ctx.handle, nm, nq, addr(lam), addr(w), len(T), addr(T), float(cutoff_THz), addr(out),
                                        addr(zpe), addr(n_excl)))
    return {"temperatures": T, "free_energy": out[:, 0].copy(), "internal_energy": out[:, 1].copy(), "entropy": out[:, 2].copy(),
            "heat_capacity": out[:, 3].copy(), "zero_point_energy": float(zpe[0]), "n_excluded": int(n_excl[0])}


def _mesh_points(mesh, qpoints, gamma_centred, time_reversal):
    if (mesh is None) == (qpoints is None):
        raise ValueError("harmonic: give either mesh or qpoints")
    if mesh is not None:
        return qmesh(mesh, gamma_centred=gamma_centred, time_reversal=time_reversal)
    q = np.ascontiguousarray(np.atleast_2d(np.asarray(qpoints, dtype=float)))
    return q, np.ones(len(q), dtype=np.int64)


def _mesh_lambda(calc, atoms, mesh, qpoints, n_super, masses, gamma_centred, time_reversal, what):
    _periodic(atoms, what)
    n = _frame(atoms)
    if n > MESH_MAX_ATOMS:
        raise ValueError(f"harmonic: the q-mesh eigensolver takes cells of at most {MESH_MAX_ATOMS} atoms (D(q) is held in LDS), "
                         f"this one has {n}")
    m = _masses(atoms, masses)
    q, w = _mesh_points(mesh, qpoints, gamma_centred, time_reversal)
    fc = _supercell_rows(calc, atoms, n_super)
    lam, _ = mesh_eigenvalues(fc, atoms, q, n_super, m, device=calc.device)
    return lam, q, w


def mesh_frequencies(calc, atoms, mesh=None, qpoints=None, n_super=5, masses=None, gamma_centred=True, time_reversal=True):
    """Phonon frequencies on a q-mesh, diagonalised on the device: ``(frequencies [nq, 3N] THz ascending, q [nq, 3] reduced,
    weights int64 [nq])``.  ``mesh`` (n1, n2, n3): ``qmesh``'s points; or explicit ``qpoints`` (weights 1).  Force constants
    and conventions are ``phonon_frequencies``'s (one device Hessian of the n_super^3 supercell, phonopy's minimum-image
    weights, ``md.resolve_masses`` rules), and so are the numbers, to rounding.  Eigenvalues only: no eigenvectors on the
    mesh.  Cells of more than 32 atoms raise ValueError."""
    lam, q, w = _mesh_lambda(calc, atoms, mesh, qpoints, n_super, masses, gamma_centred, time_reversal, "mesh_frequencies")
    return eigenvalues_to_frequencies(lam), q, w


def density_of_states(calc, atoms, mesh, n_super=5, masses=None, sigma=None, frequencies=None, n_samples=401, edges=None,
                      n_bins=100, cutoff_THz=1e-3, gamma_centred=True, time_reversal=True):
    """
    Phonon density of states on a q-mesh, all on the device.  dict:
      ``frequencies`` [n_samples] THz   the sample points (given, or evenly spaced from min(f) - 6 sigma to max(f) + 6 sigma)
      ``dos`` [n_samples]               Gaussian-smeared states per THz per cell (integral: 3N); ``sigma`` THz, default 1/100 of
                                        the largest frequency
      ``edges`` [n_bins + 1], ``counts`` int64 [n_bins]   weighted histogram of the mode frequencies (numpy's bin rule; Sigma
                                        counts = 3N n1 n2 n3 when the edges cover every mode)
      ``n_imaginary``                   summed q-weight of the modes below -cutoff_THz; anything non-zero also raises a
                                        RuntimeWarning: the structure is dynamically unstable
      ``sigma``, ``qpoints``, ``weights``, ``mode_frequencies`` [nq, 3N]
    Gaussian smearing where phonopy's default is the tetrahedron method; no point-group reduction of the mesh (time reversal
    only); the projected DOS is ``projected_dos``.
    """
    lam, q, w = _mesh_lambda(calc, atoms, mesh, None, n_super, masses, gamma_centred, time_reversal, "density_of_states")
    f = eigenvalues_to_frequencies(lam)
    f_max = max(float(np.abs(f).max()), 1e-6)
    sigma = f_max / 100.0 if sigma is None else float(sigma)
    if not sigma > 0:
        raise ValueError("harmonic.density_of_states: sigma must be positive")
    if frequencies is None:
        frequencies = np.linspace(float(f.min()) - 6 * sigma, float(f.max()) + 6 * sigma, int(n_samples))
    if edges is None:
        pad = 1e-9 * f_max
        edges = np.linspace(min(float(f.min()), 0.0) - pad, float(f.max()) + pad, int(n_bins) + 1)
    edges = np.asarray(edges, dtype=float)
    counts, dos = dos_from_eigenvalues(lam, w, edges=edges, samples=frequencies, sigma=sigma, device=calc.device)
    n_imag = int((w[:, None] * (f < -float(cutoff_THz))).sum())
    if n_imag:
        warnings.warn(f"harmonic.density_of_states: {n_imag} imaginary mode(s) on the mesh (lowest {f.min():.4g} THz): the "
                      "structure is dynamically unstable", RuntimeWarning)
    return {"frequencies": np.asarray(frequencies, dtype=float), "dos": dos, "edges": edges, "counts": counts,
            "n_imaginary": n_imag, "sigma": sigma, "qpoints": q, "weights": w, "mode_frequencies": f}


def thermal_properties(calc, atoms, temperatures, mesh, n_super=5, masses=None, cutoff_THz=1e-3, gamma_centred=True,
                       time_reversal=True):
    """
    Harmonic thermodynamics of the crystal from a q-mesh, all on the device.  dict of arrays per temperature (K):
    ``free_energy``, ``internal_energy`` (eV per cell), ``entropy``, ``heat_capacity`` (eV / K per cell), with ``temperatures``,
    ``zero_point_energy`` (eV per cell), ``n_excluded`` -- the summed q-weight of the modes with f <= cutoff_THz (the three
    acoustic modes at Gamma; imaginary modes too), which are left out of every sum -- and ``n_imaginary`` (modes below
    -cutoff_THz; non-zero raises a RuntimeWarning).  Units differ from phonopy's (kJ / mol, J / K / mol): eV per cell here.
    No quasi-harmonic volume loop.
    """
    lam, q, w = _mesh_lambda(calc, atoms, mesh, None, n_super, masses, gamma_centred, time_reversal, "thermal_properties")
    res = thermo_from_eigenvalues(lam, temperatures, w, cutoff_THz=cutoff_THz, device=calc.device)
    f = eigenvalues_to_frequencies(lam)
    n_imag = int((w[:, None] * (f < -float(cutoff_THz))).sum())
    if n_imag:
        warnings.warn(f"harmonic.thermal_properties: {n_imag} imaginary mode(s) on the mesh (lowest {f.min():.4g} THz) are left "
                      "out of the sums: the structure is dynamically unstable", RuntimeWarning)
    res["n_imaginary"] = n_imag
    return res


# ------------------------------------------------------------------------------- eigenvectors on the q-mesh (device)
# DESIGN.md section 3.23.  uf3_phonon_mesh_vec returns V(q) and the group velocities beside the eigenvalues (the same bits as
# uf3_phonon_mesh); uf3_phonon_pdos and uf3_phonon_tdisp reduce V over the mesh.  A mesh whose vectors do not fit in one
# allocation goes through in q-slabs of ``vector_slab(3N)`` points, a function of 3N alone: every q is independent in the
# eigensolver, and the reductions add their slabs' partial results in slab order, so nothing depends on free memory.
VEC_MAX_ATOMS = 21                     # uf3_phonon_mesh_vec: V beside D(q) in LDS, 32 (3N)^2 bytes (3N = 63: 127 KB of 160)
VEC_SLAB_BYTES = 1 << 28               # eigenvectors of one q-slab: at most 256 MiB


def vector_slab(n_modes):
    """q-points per slab of the eigenvector routes: ``2^28 // (16 n_modes^2)`` -- 256 MiB of complex vectors."""
    return max(1, VEC_SLAB_BYTES // (16 * int(n_modes) ** 2))


def _vec_limit(n):
    if n > VEC_MAX_ATOMS:
        raise ValueError(f"harmonic: eigenvectors on the q-mesh take cells of at most {VEC_MAX_ATOMS} atoms (V is held beside D(q) "
                         f"in LDS), this one has {n}")


def _mesh_vec_call(ctx, n, n_sc, flat, inv_sqrt_m, terms, w, q, cell, cutoff, want_vec, want_vel):
    lam = np.empty((len(q), 3 * n))
    status = np.empty(len(q), dtype=np.int32)
    vec = np.empty((len(q), 3 * n, 3 * n), dtype=np.complex128) if want_vec else None
    vel = np.empty((len(q), 3 * n, 3)) if want_vel else None
    addr = _lib._addr
    ctx.check(ctx.lib.uf3_phonon_mesh_vec(ctx.handle, n, n_sc, addr(flat), addr(inv_sqrt_m), len(terms), addr(terms), addr(w), len(q),
                                          addr(q), addr(lam), addr(status), addr(cell), float(cutoff), addr(vec), addr(vel)))
    if np.any(status < 0):
        bad = np.flatnonzero(status < 0)
        raise RuntimeError(f"harmonic.mesh_eigenvectors: the Jacobi iteration did not converge within its sweep cap at {len(bad)} "
                           f"q-point(s), the first q = {q[bad[0]].tolist()}")
    return lam, status, vec, vel


def _mesh_vec_setup(fc_rows, atoms, qpoints, n_super, masses, what):
    n = _frame(atoms)
    _vec_limit(n)
    fc = np.asarray(fc_rows, dtype=float)
    n_sc = n * int(n_super) ** 3
    if fc.shape != (n, n_sc, 3, 3):
        raise ValueError(f"harmonic.{what}: fc_rows must be [{n}, {n_sc}, 3, 3], got {fc.shape}")
    q = np.ascontiguousarray(np.atleast_2d(np.asarray(qpoints, dtype=float)))
    if q.ndim != 2 or q.shape[1] != 3 or len(q) < 1:
        raise ValueError(f"harmonic.{what}: qpoints must be [nq, 3] with nq >= 1")
    m = np.asarray(masses, dtype=float).reshape(-1)
    if m.shape != (n,) or np.any(m <= 0):
        raise ValueError(f"harmonic.{what}: one positive mass per atom")
    flat = np.ascontiguousarray(fc.transpose(0, 2, 1, 3).reshape(3 * n, 3 * n_sc))
    inv_sqrt_m = np.ascontiguousarray(1.0 / np.sqrt(m))
    terms, w = image_terms(atoms, n_super)
    cell = np.ascontiguousarray(np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3))
    return n, n_sc, flat, inv_sqrt_m, terms, w, q, cell


def mesh_eigenvectors(fc_rows, atoms, qpoints, n_super, masses, velocities=False, device=None, cutoff_THz=1e-3, vectors=True):
    """Eigenpairs of D(q) on the device (``uf3_phonon_mesh_vec``): ``(lam [nq, 3N] ascending, vec [nq, 3N, 3N] complex)`` and,
    with ``velocities=True``, ``vel [nq, 3N, 3]`` (THz A; 1 THz A = 100 m / s).  Arguments as for ``mesh_eigenvalues``, whose
    ``lam`` this returns bit for bit; ``vec[k][:, s]`` is an orthonormal eigenvector of ``lam[k, s]`` (row 3 i + alpha: atom i,
    Cartesian alpha; the convention of ``dynamical_matrices``, without the phase exp(2 pi i q.r_i)).  vel = d f / d k by
    Hellmann-Feynman, k the Cartesian wave vector without 2 pi; modes with |f| <= ``cutoff_THz`` get 0.  Inside a degenerate
    cluster of modes any orthonormal basis is a correct answer, and the velocities of its members depend on the basis the
    Jacobi sweeps ended in: only the cluster's sum is defined.  ``vectors=False`` (with velocities) leaves vec out (None).
    The q-points go through in slabs of ``vector_slab(3N)`` = 2^28 // (16 (3N)^2) points (256 MiB of vectors); the result
    does not depend on the cut.  Cells of more than ``VEC_MAX_ATOMS`` = 21 atoms raise ValueError, a q-point that does not
    converge RuntimeError."""
    if not vectors and not velocities:
        raise ValueError("harmonic.mesh_eigenvectors: nothing asked for (vectors=False without velocities)")
    if not float(cutoff_THz) >= 0:
        raise ValueError("harmonic.mesh_eigenvectors: cutoff_THz must be >= 0")
    n, n_sc, flat, ism, terms, w, q, cell = _mesh_vec_setup(fc_rows, atoms, qpoints, n_super, masses, "mesh_eigenvectors")
    ctx = _mesh_context(device)
    slab = vector_slab(3 * n)
    parts = [_mesh_vec_call(ctx, n, n_sc, flat, ism, terms, w, np.ascontiguousarray(q[k:k + slab]), cell, cutoff_THz, vectors,
                            velocities) for k in range(0, len(q), slab)]
    lam, _, vec, vel = (parts[0] if len(parts) == 1 else
                        tuple(None if parts[0][j] is None else np.concatenate([p[j] for p in parts]) for j in range(4)))
    return (lam, vec, vel) if velocities else (lam, vec)


def pdos_from_eigenvectors(lam, vec, weights=None, samples=None, sigma=None, device=None):
    """``uf3_phonon_pdos``: [n_modes, n_samples], the Gaussian-smeared DOS of every channel 3 i + alpha, from lam [nq, n_modes]
    and vec [nq, n_modes, n_modes] as ``mesh_eigenvectors`` returns them; normalised like ``dos_from_eigenvalues``."""
    lam = np.ascontiguousarray(lam, dtype=float)
    vec = np.ascontiguousarray(vec, dtype=np.complex128)
    if lam.ndim != 2 or lam.size == 0 or vec.shape != lam.shape + (lam.shape[1],):
        raise ValueError("harmonic.pdos_from_eigenvectors: lam must be [nq, n_modes] and vec [nq, n_modes, n_modes]")
    nq, nm = lam.shape
    w = _weights(weights, nq)
    samples = np.ascontiguousarray(samples, dtype=float).reshape(-1)
    if sigma is None or not float(sigma) > 0:
        raise ValueError("harmonic.pdos_from_eigenvectors: sigma must be positive")
    out = np.zeros((nm, len(samples)))
    ctx = _mesh_context(device)
    addr = _lib._addr
    ctx.check(ctx.lib.uf3_phonon_pdos(ctx.handle, nm, nq, addr(lam), addr(vec), addr(w), len(samples), addr(samples), float(sigma),
                                      addr(out)))
    return out


def tdisp_from_eigenvectors(lam, vec, masses, temperatures, weights=None, cutoff_THz=1e-3, device=None):
    """``uf3_phonon_tdisp``: ``(U6 [nT, N, 6] in A^2 -- xx, yy, zz, yz, xz, xy --, n_excluded)`` from lam [nq, 3N], vec
    [nq, 3N, 3N] and per-atom masses (amu)."""
    lam = np.ascontiguousarray(lam, dtype=float)
    vec = np.ascontiguousarray(vec, dtype=np.complex128)
    if lam.ndim != 2 or lam.size == 0 or lam.shape[1] % 3 or vec.shape != lam.shape + (lam.shape[1],):
        raise ValueError("harmonic.tdisp_from_eigenvectors: lam must be [nq, 3N] and vec [nq, 3N, 3N]")
    nq, nm = lam.shape
    m = np.asarray(masses, dtype=float).reshape(-1)
    if m.shape != (nm // 3,) or np.any(m <= 0):
        raise ValueError("harmonic.tdisp_from_eigenvectors: one positive mass per atom")
    w = _weights(weights, nq)
    T = np.ascontiguousarray(np.atleast_1d(np.asarray(temperatures, dtype=float)).reshape(-1))
    if len(T) < 1 or not np.all(np.isfinite(T)) or np.any(T < 0):
        raise ValueError("harmonic.tdisp_from_eigenvectors: temperatures must be finite and >= 0")
    if not float(cutoff_THz) >= 0:
        raise ValueError("harmonic.tdisp_from_eigenvectors: cutoff_THz must be >= 0")
    ism = np.ascontiguousarray(1.0 / np.sqrt(m))
    out = np.empty((len(T), nm // 3, 6))
    n_excl = np.empty(1, dtype=np.int64)
    ctx = _mesh_context(device)
    addr = _lib._addr
    ctx.check(ctx.lib.uf3_phonon_tdisp(ctx.handle, nm // 3, nq, addr(lam), addr(vec), addr(w), addr(ism), len(T), addr(T),
                                       float(cutoff_THz), addr(out), addr(n_excl)))
    return out, int(n_excl[0])


def _slabs(calc, atoms, mesh, n_super, masses, gamma_centred, time_reversal, what):
    """(generator of (lam, vec, w) per q-slab; q, w, m): one Hessian call, then ``mesh_eigenvectors`` slab by slab."""
    _periodic(atoms, what)
    n = _frame(atoms)
    _vec_limit(n)
    m = _masses(atoms, masses)
    q, w = _mesh_points(mesh, None, gamma_centred, time_reversal)
    fc = _supercell_rows(calc, atoms, n_super)
    slab = vector_slab(3 * n)

    def gen():
        for k in range(0, len(q), slab):
            lam, vec = mesh_eigenvectors(fc, atoms, q[k:k + slab], n_super, m, device=calc.device)
            yield lam, vec, w[k:k + slab]
    return gen, q, w, m


def group_pdos(channels, atoms, by):
    """Sum the channel-resolved PDOS [3N, n_samples] into groups: ``(pdos [n_groups, n_samples], labels)``.  ``by="channel"``: as
    is, labels (i, "x" | "y" | "z"); ``"atom"``: the three channels of an atom, labels the atom indices; ``"species"``: the
    atoms of a chemical symbol in order of first appearance, labels the symbols (atomic numbers when the frame has none)."""
    channels = np.asarray(channels, dtype=float)
    n = channels.shape[0] // 3
    if by == "channel":
        return channels, [(i, "xyz"[a]) for i in range(n) for a in range(3)]
    per_atom = channels.reshape(n, 3, -1).sum(axis=1)
    if by == "atom":
        return per_atom, list(range(n))
    if by == "species":
        try:
            names = list(atoms.get_chemical_symbols())
        except AttributeError:
            names = [int(z) for z in atoms.get_atomic_numbers()]
        labels = list(dict.fromkeys(names))
        return np.array([per_atom[[k for k, s in enumerate(names) if s == lab]].sum(axis=0) for lab in labels]), labels
    raise ValueError(f"harmonic.projected_dos: by must be 'atom', 'species' or 'channel', got {by!r}")


def projected_dos(calc, atoms, mesh, n_super=5, masses=None, sigma=None, frequencies=None, n_samples=401, cutoff_THz=1e-3,
                  gamma_centred=True, time_reversal=True, by="atom"):
    """
    Projected phonon density of states on a q-mesh, all on the device.  dict:
      ``frequencies`` [n_samples] THz, ``sigma``    as ``density_of_states``
      ``pdos`` [n_groups, n_samples]                g_c(f) = Sigma_q w_q Sigma_s |V_cs|^2 gaussian(f - f_s) / Sigma_q w_q summed over the
                                                    channels of a group; ``by``: "atom", "species" or "channel" (``group_pdos``)
      ``labels``                                    one per group
      ``dos`` [n_samples]                           the total: the sum of the groups (V is unitary)
      ``channels`` [3N, n_samples], ``n_imaginary``, ``qpoints``, ``weights``, ``mode_frequencies``
    Inside a degenerate cluster the vectors are one orthonormal basis of many, which the PDOS does not see: such modes share
    their frequency.  Meshes go through in q-slabs of ``vector_slab(3N)`` = 2^28 // (16 (3N)^2) points, added in slab order.
    Cells of more than 21 atoms raise ValueError.
    """
    if by not in ("atom", "species", "channel"):
        raise ValueError(f"harmonic.projected_dos: by must be 'atom', 'species' or 'channel', got {by!r}")
    gen, q, w, _ = _slabs(calc, atoms, mesh, n_super, masses, gamma_centred, time_reversal, "projected_dos")
    slabs = list(gen()) if len(q) <= vector_slab(3 * _frame(atoms)) else None
    # the sample range needs every frequency first: with more than one slab the vectors are computed twice, not kept
    f = eigenvalues_to_frequencies(np.concatenate([s[0] for s in (slabs if slabs is not None else gen())]))
    f_max = max(float(np.abs(f).max()), 1e-6)
    sigma = f_max / 100.0 if sigma is None else float(sigma)
    if not sigma > 0:
        raise ValueError("harmonic.projected_dos: sigma must be positive")
    if frequencies is None:
        frequencies = np.linspace(float(f.min()) - 6 * sigma, float(f.max()) + 6 * sigma, int(n_samples))
    frequencies = np.ascontiguousarray(frequencies, dtype=float)
    wsum = float(w.sum())
    channels = None
    for lam, vec, ws in (slabs if slabs is not None else gen()):
        part = pdos_from_eigenvectors(lam, vec, ws, samples=frequencies, sigma=sigma, device=calc.device)
        part = part if len(ws) == len(w) else part * (float(ws.sum()) / wsum)
        channels = part if channels is None else channels + part
    pdos, labels = group_pdos(channels, atoms, by)
    n_imag = int((w[:, None] * (f < -float(cutoff_THz))).sum())
    if n_imag:
        warnings.warn(f"harmonic.projected_dos: {n_imag} imaginary mode(s) on the mesh (lowest {f.min():.4g} THz): the "
                      "structure is dynamically unstable", RuntimeWarning)
    return {"frequencies": frequencies, "pdos": pdos, "labels": labels, "dos": channels.sum(axis=0), "channels": channels,
            "n_imaginary": n_imag, "sigma": sigma, "qpoints": q, "weights": w, "mode_frequencies": f}


def voigt6_to_tensors(u6):
    """[..., 6] (xx, yy, zz, yz, xz, xy) -> symmetric [..., 3, 3]."""
    u6 = np.asarray(u6, dtype=float)
    U = np.empty(u6.shape[:-1] + (3, 3))
    for k, (a, b) in enumerate(_VOIGT):
        U[..., a, b] = U[..., b, a] = u6[..., k]
    return U


def thermal_displacements(calc, atoms, temperatures, mesh, n_super=5, masses=None, cutoff_THz=1e-3, gamma_centred=True,
                          time_reversal=True):
    """
    Mean-square thermal displacement tensors (Debye-Waller factors) in the harmonic approximation, on the device.  dict:
      ``U`` [n_T, N, 3, 3] A^2    U_i^{ab}(T) = (1 / Sigma w_q) Sigma_q w_q Sigma_s E_s(T) / (m_i lam_s) Re(V_{3i+a,s} conj V_{3i+b,s}),
                                  E_s = h f_s (1/2 + 1 / (e^x - 1)), x = h f_s / k_B T; T = 0: the zero-point motion
      ``u_iso`` [n_T, N] A^2      tr U / 3
      ``n_excluded``              summed q-weight of the modes with f <= cutoff_THz, left out (Gamma's acoustic modes, whose
                                  term diverges; imaginary modes too), ``n_imaginary`` as ``thermal_properties``
      ``temperatures``
    Meshes go through in q-slabs of ``vector_slab(3N)`` = 2^28 // (16 (3N)^2) points, added in slab order.  Cells of more than
    21 atoms raise ValueError.
    """
    gen, q, w, m = _slabs(calc, atoms, mesh, n_super, masses, gamma_centred, time_reversal, "thermal_displacements")
    T = np.ascontiguousarray(np.atleast_1d(np.asarray(temperatures, dtype=float)).reshape(-1))
    wsum = float(w.sum())
    u6, n_excl, lams = None, 0, []
    for lam, vec, ws in gen():
        part, nx = tdisp_from_eigenvectors(lam, vec, m, T, ws, cutoff_THz=cutoff_THz, device=calc.device)
        part = part if len(ws) == len(w) else part * (float(ws.sum()) / wsum)
        u6 = part if u6 is None else u6 + part
        n_excl += nx
        lams.append(lam)
    f = eigenvalues_to_frequencies(np.concatenate(lams))
    n_imag = int((w[:, None] * (f < -float(cutoff_THz))).sum())
    if n_imag:
        warnings.warn(f"harmonic.thermal_displacements: {n_imag} imaginary mode(s) on the mesh (lowest {f.min():.4g} THz) are left "
                      "out of the sums: the structure is dynamically unstable", RuntimeWarning)
    U = voigt6_to_tensors(u6)
    return {"temperatures": T, "U": U, "u_iso": np.trace(U, axis1=-2, axis2=-1) / 3.0, "n_excluded": int(n_excl),
            "n_imaginary": n_imag}


def group_velocities(calc, atoms, qpoints, n_super=5, masses=None, cutoff_THz=1e-3):
    """Phonon group velocities at reduced wave vectors ``qpoints`` [nq, 3]: ``(frequencies [nq, 3N] THz ascending, velocities
    [nq, 3N, 3] THz A)``, v = d f / d k with k the Cartesian wave vector without 2 pi (1 THz A = 100 m / s), from the device's
    eigenvectors by Hellmann-Feynman (``mesh_eigenvectors``; no finite differences).  Modes with |f| <= ``cutoff_THz`` get 0
    (Gamma's acoustic modes, where the slope is not defined).  Inside a degenerate cluster of modes only the sum of the
    members' velocities is defined; they are not diagonalised there."""
    _periodic(atoms, "group_velocities")
    m = _masses(atoms, masses)
    _vec_limit(_frame(atoms))
    fc = _supercell_rows(calc, atoms, n_super)
    lam, _, vel = mesh_eigenvectors(fc, atoms, qpoints, n_super, m, velocities=True, device=calc.device, cutoff_THz=cutoff_THz,
                                    vectors=False)
    return eigenvalues_to_frequencies(lam), vel


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
