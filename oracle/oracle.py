"""
ctypes front-end of the CPU restatement (``oracle/uf3_oracle.c``) plus the NumPy
restatement of the normal-equation fit.  TEST INFRASTRUCTURE ONLY: imported by
``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s cpu_baseline leg.

The basis description is read from any object exposing the reference's
``BSplineBasis`` attribute names (``knots_map``, ``symmetry``, ``template_mask``,
``flat_weights``, ``leading_trim`` ...), so the same wrapper runs on the
reference's own class (golden capture) and on ``uf3_amd``'s.

The C source builds twice: ``libuf3oracle.so`` (fp64; ``featurize``, ``evaluate``) and ``libuf3oracle_x.so`` (``long double``
values on fp64 decisions; ``featurize_x``, ``evaluate_x``, ``hessian_x``, ``site_terms_x``, ``site_rows_x``, ``mc_delta_x``, which also return the magnitude M of every
entry -- see uf3_oracle.c and tests/_precision.py).
"""
import ctypes as C
import os
import subprocess
import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_LIB_X = None

_SYMBOLS = ("X H He Li Be B C N O F Ne Na Mg Al Si P S Cl Ar K Ca Sc Ti V Cr Mn Fe Co Ni Cu Zn Ga "
            "Ge As Se Br Kr Rb Sr Y Zr Nb Mo Tc Ru Rh Pd Ag Cd In Sn Sb Te I Xe Cs Ba La Ce Pr Nd "
            "Pm Sm Eu Gd Tb Dy Ho Er Tm Yb Lu Hf Ta W Re Os Ir Pt Au Hg Tl Pb Bi Po At Rn Fr Ra Ac "
            "Th Pa U Np Pu Am Cm Bk Cf Es Fm Md No Lr Rf Db Sg Bh Hs Mt Ds Rg Cn Nh Fl Mc Lv Ts "
            "Og").split()
_Z = {s: z for z, s in enumerate(_SYMBOLS)}


class _Spec(C.Structure):
    _fields_ = [("n_species", C.c_int), ("species_z", C.c_void_p),
                ("n_pairs", C.c_int), ("pair_z", C.c_void_p), ("pair_nk", C.c_void_p),
                ("pair_knots", C.c_void_p), ("pair_rmin", C.c_void_p), ("pair_rmax", C.c_void_p),
                ("pair_col", C.c_void_p),
                ("lead2", C.c_int), ("trail2", C.c_int), ("lead3", C.c_int), ("trail3", C.c_int),
                ("n_trios", C.c_int), ("trio_z", C.c_void_p), ("trio_nk", C.c_void_p),
                ("trio_knots", C.c_void_p), ("trio_sym", C.c_void_p), ("trio_col", C.c_void_p),
                ("trio_ncol", C.c_void_p), ("trio_mask", C.c_void_p), ("trio_w", C.c_void_p),
                ("n_feat", C.c_int), ("r_cut", C.c_double)]


class _Frame(C.Structure):
    _fields_ = [("n_atoms", C.c_int), ("pos", C.c_void_p), ("z", C.c_void_p),
                ("cell", C.c_void_p), ("pbc", C.c_void_p)]


def build(force=False, name="libuf3oracle.so"):
    """Compile libuf3oracle.so (or ``name``) next to the source (gcc, seconds)."""
    so = os.path.join(_HERE, name)
    src = os.path.join(_HERE, "uf3_oracle.c")
    if force or not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", _HERE, "-B", name],
                              stdout=subprocess.DEVNULL)
    return so


def _load(name):
    so = C.CDLL(build(name=name))
    for f in ("uf3o_featurize", "uf3o_featurize_x", "uf3o_eval", "uf3o_eval_virial", "uf3o_eval_x", "uf3o_real_mant_dig",
              "uf3o_hessian_x", "uf3o_site_terms_x", "uf3o_site_rows_x", "uf3o_mc_delta_x", "uf3o_mc_terms_x"):
        getattr(so, f).restype = C.c_int
    so.uf3o_supercell.restype = C.c_int64
    return so


def lib():
    global _LIB
    if _LIB is None:
        _LIB = _load("libuf3oracle.so")
    return _LIB


def lib_x():
    """The extended build of the same source (``real`` = long double, 64-bit mantissa).  Only its ``*_x`` entries are called:
    its arrays of values are ``np.longdouble``."""
    global _LIB_X
    if _LIB_X is None:
        if np.finfo(np.longdouble).nmant + 1 < 64 or np.dtype(np.longdouble).itemsize != C.sizeof(C.c_longdouble):
            raise RuntimeError("np.longdouble is not the C long double with a 64-bit mantissa on this platform")
        _LIB_X = _load("libuf3oracle_x.so")
        if _LIB_X.uf3o_real_mant_dig() < 64:
            raise RuntimeError("libuf3oracle_x.so was built without an extended type")
    return _LIB_X


def mant_dig(extended=True):
    """Mantissa bits of the arithmetic type of the extended (or the fp64) build."""
    return int((lib_x() if extended else lib()).uf3o_real_mant_dig())


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class OracleBasis:
    """Flat C view of a BSplineBasis-like object (keeps the arrays alive)."""

    def __init__(self, basis):
        self.basis = basis
        cs = basis.chemical_system
        els = list(cs.element_list)
        self.species_z = np.array([_Z[e] for e in els], dtype=np.int32)
        sizes, offsets = basis.get_interaction_partitions()
        pairs = list(cs.interactions_map[2])
        self.pair_z = np.array([[_Z[a], _Z[b]] for a, b in pairs], dtype=np.int32).reshape(-1, 2)
        pk = [np.asarray(basis.knots_map[p], dtype=np.float64) for p in pairs]
        self.pair_nk = np.array([len(k) for k in pk], dtype=np.int32)
        self.pair_knots = np.concatenate(pk) if pk else np.zeros(0)
        self.pair_rmin = np.array([float(basis.r_min_map[p]) for p in pairs])
        self.pair_rmax = np.array([float(basis.r_max_map[p]) for p in pairs])
        self.pair_col = np.array([int(offsets[p]) for p in pairs], dtype=np.int32)
        trios = list(cs.interactions_map.get(3, [])) if cs.degree > 2 else []
        self.trios = trios
        self.pairs = pairs
        self.trio_z = np.array([[_Z[a], _Z[b], _Z[c]] for a, b, c in trios],
                               dtype=np.int32).reshape(-1, 3)
        tk = [[np.asarray(k, dtype=np.float64) for k in basis.knots_map[t]] for t in trios]
        self.trio_nk = np.array([[len(k) for k in ks] for ks in tk], dtype=np.int32).reshape(-1, 3)
        self.trio_knots = (np.concatenate([k for ks in tk for k in ks]) if trios else np.zeros(0))
        self.trio_sym = np.array([basis.symmetry[t] for t in trios], dtype=np.int32)
        self.trio_col = np.array([int(offsets[t]) for t in trios], dtype=np.int32)
        self.trio_ncol = np.array([int(sizes[t]) for t in trios], dtype=np.int32)
        self.trio_mask = (np.concatenate([np.asarray(basis.template_mask[t], dtype=np.int64)
                                          for t in trios]) if trios else np.zeros(0, np.int64))
        self.trio_w = (np.concatenate([np.asarray(basis.flat_weights[t], dtype=np.float64)
                                       for t in trios]) if trios else np.zeros(0))
        self.n_feat = int(np.sum(basis.get_feature_partition_sizes()))
        self.grid_shapes = [tuple(int(n) - 4 for n in row) for row in self.trio_nk]
        s = _Spec()
        s.n_species = len(els)
        s.species_z = _ptr(self.species_z)
        s.n_pairs = len(pairs)
        s.pair_z, s.pair_nk, s.pair_knots = _ptr(self.pair_z), _ptr(self.pair_nk), _ptr(self.pair_knots)
        s.pair_rmin, s.pair_rmax, s.pair_col = _ptr(self.pair_rmin), _ptr(self.pair_rmax), _ptr(self.pair_col)
        s.lead2, s.trail2 = int(basis.leading_trim[2]), int(basis.trailing_trim[2])
        s.lead3, s.trail3 = int(basis.leading_trim.get(3, 0)), int(basis.trailing_trim.get(3, 0))
        s.n_trios = len(trios)
        s.trio_z, s.trio_nk, s.trio_knots = _ptr(self.trio_z), _ptr(self.trio_nk), _ptr(self.trio_knots)
        s.trio_sym, s.trio_col, s.trio_ncol = _ptr(self.trio_sym), _ptr(self.trio_col), _ptr(self.trio_ncol)
        s.trio_mask, s.trio_w = _ptr(self.trio_mask), _ptr(self.trio_w)
        s.n_feat = self.n_feat
        s.r_cut = float(basis.r_cut)
        self.spec = s


class _FrameView:
    def __init__(self, atoms):
        self.pos = np.ascontiguousarray(atoms.get_positions(), dtype=np.float64)
        self.z = np.ascontiguousarray(atoms.get_atomic_numbers(), dtype=np.int32)
        cell = atoms.get_cell()
        self.cell = np.ascontiguousarray(np.array(cell, dtype=np.float64).reshape(3, 3))
        pbc = np.zeros(3, dtype=np.int32)
        pbc[:] = np.asarray(atoms.get_pbc() if hasattr(atoms, "get_pbc") else atoms.pbc)
        self.pbc = pbc
        f = _Frame()
        f.n_atoms = len(self.z)
        f.pos, f.z, f.cell, f.pbc = _ptr(self.pos), _ptr(self.z), _ptr(self.cell), _ptr(self.pbc)
        self.c = f


def _rows_x(so, dtype, ob, atoms, virial, pieces):
    fv = _FrameView(atoms)
    n, F = fv.c.n_atoms, ob.n_feat
    val = {"xe": np.zeros(F, dtype), "xf": np.zeros((n, 3, F), dtype), "xv": np.zeros((6, F), dtype) if virial else None}
    mag = {k: (np.zeros(v.shape) if v is not None else None) for k, v in val.items()}
    pair_cnt, n3_cnt = np.zeros(max(1, ob.spec.n_pairs), dtype=np.int64), np.zeros(1, dtype=np.int64)
    rc = so.uf3o_featurize_x(C.byref(ob.spec), C.byref(fv.c), _ptr(val["xe"]), _ptr(val["xf"]), _ptr(val["xv"]),
                             _ptr(mag["xe"]), _ptr(mag["xf"]), _ptr(mag["xv"]), C.c_int(int(pieces)), _ptr(pair_cnt),
                             _ptr(n3_cnt))
    if rc:
        raise RuntimeError(f"uf3o_featurize_x rc={rc}")
    if not virial:
        del val["xv"], mag["xv"]
    val["pair_cnt"], val["n3_cnt"] = pair_cnt[:ob.spec.n_pairs].copy(), int(n3_cnt[0])
    return val, mag


def featurize_x(ob, atoms, virial=False, extended=True, pieces=False):
    """
    The rows of ``featurize`` from the extended build: ``(values, magnitudes)``, two dicts with keys ``xe`` [F], ``xf`` [N,3,F]
    and, with ``virial=True``, ``xv`` [6,F] (the strain derivative of the energy row, Voigt, the convention of
    ``evaluate(virial=True)``).  Values are ``np.longdouble``; a magnitude M (float64) is the first-order running error bound of
    its entry (uf3_oracle.c): a result computed in fp64 lies within a modest multiple of ``2**-53 * M`` of the value.
    ``values`` also holds ``pair_cnt`` [P] and ``n3_cnt``, the numbers of pairs and 3-body list entries summed.
    ``extended=False`` runs the same entry of the fp64 build (values float64, the same magnitudes to rounding).
    ``pieces=True`` widens the magnitudes of the 3-body columns to those of leg functions evaluated from local cubic pieces in
    powers of the distance from the interval's lower knot (uf3_oracle.c: piece_abs), for the routes that do so.
    """
    if extended:
        return _rows_x(lib_x(), np.longdouble, ob, atoms, virial, pieces)
    return _rows_x(lib(), np.float64, ob, atoms, virial, pieces)


def evaluate_x(ob, atoms, coefficients, virial=True, extended=True, forces=True):
    """``evaluate`` from the extended build: ``(values, magnitudes)``, dicts with keys ``e`` (scalar), ``f`` [N,3] and, with
    ``virial=True``, ``v`` [6]; see ``featurize_x``.  ``forces=False`` (with ``virial=False``): the energy alone, ``f`` None."""
    so, dtype = (lib_x(), np.longdouble) if extended else (lib(), np.float64)
    c1, c2, c3 = split_coefficients(ob, coefficients)
    fv = _FrameView(atoms)
    e, f, v = np.zeros(1, dtype), np.zeros((fv.c.n_atoms, 3), dtype) if forces else None, np.zeros(6, dtype) if virial else None
    me, mf, mv = np.zeros(1), np.zeros((fv.c.n_atoms, 3)) if forces else None, np.zeros(6) if virial else None
    rc = so.uf3o_eval_x(C.byref(ob.spec), C.byref(fv.c), _ptr(c1), _ptr(c2), _ptr(c3), _ptr(e), _ptr(f), _ptr(v),
                        _ptr(me), _ptr(mf), _ptr(mv))
    if rc:
        raise RuntimeError(f"uf3o_eval_x rc={rc}")
    val, mag = {"e": e[0], "f": f}, {"e": me[0], "f": mf}
    if virial:
        val["v"], mag["v"] = v, mv
    return val, mag


def supercell_radius(ob, atoms):
    """The radius the supercell of ``hessian_x``, ``site_terms_x`` and ``site_rows_x`` is built for: the basis' ``r_cut``, plus
    how far the farthest atom lies from its image inside the cell.  Those entries describe the frame with every atom counted as
    its image inside the cell (as the device entries they check do), while the supercell tiles the positions as given around
    the cell: the wider radius keeps every image that a real atom's terms reach.  A frame inside its cell: ``r_cut`` itself."""
    fv = _FrameView(atoms)
    pad = 0.0
    if fv.pbc.any() and abs(np.linalg.det(fv.cell)) > 0:
        frac = fv.pos @ np.linalg.inv(fv.cell)
        out = np.where(fv.pbc.astype(bool)[None, :], np.floor(frac + 1e-9 * (frac < 0) - 1e-9 * (frac >= 1)), 0.0)
        pad = float(np.linalg.norm(out @ fv.cell, axis=1).max()) if len(out) else 0.0
    return float(ob.basis.r_cut) + pad


def _kind(extended):
    return (lib_x(), np.longdouble) if extended else (lib(), np.float64)


def hessian_x(ob, atoms, coefficients, strain=True, extended=True):
    """Second derivatives of ``evaluate``'s energy (uf3_hessian.h) from the extended build: ``(values, magnitudes)``, dicts with
    keys ``H`` [3N,3N] and, with ``strain=True``, ``mixed`` [3N,6] and ``born`` [6,6]; see ``featurize_x``."""
    so, dtype = _kind(extended)
    c1, c2, c3 = split_coefficients(ob, coefficients)
    fv = _FrameView(atoms)
    n3 = 3 * fv.c.n_atoms
    val = {"H": np.zeros((n3, n3), dtype), "mixed": np.zeros((n3, 6), dtype) if strain else None,
           "born": np.zeros((6, 6), dtype) if strain else None}
    mag = {k: (np.zeros(v.shape) if v is not None else None) for k, v in val.items()}
    rc = so.uf3o_hessian_x(C.byref(ob.spec), C.byref(fv.c), _ptr(c1), _ptr(c2), _ptr(c3), C.c_double(supercell_radius(ob, atoms)),
                           _ptr(val["H"]), _ptr(val["mixed"]), _ptr(val["born"]), _ptr(mag["H"]), _ptr(mag["mixed"]),
                           _ptr(mag["born"]))
    if rc:
        raise RuntimeError(f"uf3o_hessian_x rc={rc}")
    if not strain:
        for d in (val, mag):
            del d["mixed"], d["born"]
    return val, mag


def site_terms_x(ob, atoms, coefficients, velocities=None, extended=True):
    """Site energies, site virials and each centre's share of the heat current's potential part (uf3_flux.h) from the extended
    build: ``(values, magnitudes)``, dicts with keys ``U`` [N], ``W`` [N,3,3] and, with ``velocities`` [N,3], ``jp`` [N,3];
    ``values["e"]`` / ``magnitudes["e"]``: the frame's energy from the same loop.  See ``featurize_x``."""
    so, dtype = _kind(extended)
    c1, c2, c3 = split_coefficients(ob, coefficients)
    fv = _FrameView(atoms)
    n = fv.c.n_atoms
    vel = None if velocities is None else np.ascontiguousarray(np.asarray(velocities, dtype=np.float64).reshape(n, 3))
    val = {"U": np.zeros(n, dtype), "W": np.zeros((n, 3, 3), dtype), "jp": np.zeros((n, 3), dtype) if vel is not None else None}
    mag = {k: (np.zeros(v.shape) if v is not None else None) for k, v in val.items()}
    e, me = np.zeros(1, dtype), np.zeros(1)
    rc = so.uf3o_site_terms_x(C.byref(ob.spec), C.byref(fv.c), _ptr(c1), _ptr(c2), _ptr(c3),
                              C.c_double(supercell_radius(ob, atoms)), _ptr(vel), _ptr(val["U"]), _ptr(val["W"]), _ptr(val["jp"]),
                              _ptr(mag["U"]), _ptr(mag["W"]), _ptr(mag["jp"]), _ptr(e), _ptr(me))
    if rc:
        raise RuntimeError(f"uf3o_site_terms_x rc={rc}")
    if vel is None:
        del val["jp"], mag["jp"]
    val["e"], mag["e"] = e[0], me[0]
    return val, mag


def site_rows_x(ob, atoms, extended=True):
    """Site rows (uf3_site_rows.h) from the extended build: ``(values, magnitudes)``, dicts with keys ``b`` [N,F] -- the energy
    row's terms credited to their centre, folded into columns as ``featurize_x`` folds them -- and ``xe`` [F], the energy row of
    the same walk.  See ``featurize_x``."""
    so, dtype = _kind(extended)
    fv = _FrameView(atoms)
    n, F = fv.c.n_atoms, ob.n_feat
    val = {"b": np.zeros((n, F), dtype), "xe": np.zeros(F, dtype)}
    mag = {"b": np.zeros((n, F)), "xe": np.zeros(F)}
    rc = so.uf3o_site_rows_x(C.byref(ob.spec), C.byref(fv.c), C.c_double(supercell_radius(ob, atoms)), _ptr(val["b"]),
                             _ptr(mag["b"]), _ptr(val["xe"]), _ptr(mag["xe"]))
    if rc:
        raise RuntimeError(f"uf3o_site_rows_x rc={rc}")
    return val, mag


MC_MODES = {"swap": 0, "transmute": 1}
MC_TERM_FIELDS = ("pass", "kind", "centre", "p1", "p2", "value", "magnitude", "distance", "legs_exchanged", "leg_fp32", "r_ij", "r_ik")


def _mc_second(mode, j_or_species):
    """the second column of a move list as int32: atom indices (swap) or atomic numbers (transmute; symbols accepted)"""
    if MC_MODES[mode] == 0:
        return np.ascontiguousarray(j_or_species, dtype=np.int32).reshape(-1)
    return np.ascontiguousarray([_Z[q] if isinstance(q, str) else int(q) for q in np.atleast_1d(j_or_species)], dtype=np.int32)


def mc_delta_x(ob, atoms, coefficients, i, j_or_species, mode, extended=True):
    """Energy differences of Monte Carlo moves on the frame's species (uf3_mc.h's definition; uf3_oracle.c: uf3o_mc_delta_x):
    ``mode`` "swap" exchanges the species of atoms ``i[k]`` and ``j_or_species[k]``, "transmute" gives atom ``i[k]`` the element
    ``j_or_species[k]`` (symbol or atomic number).  Returns ``(dE, M)``, both [n_moves]: dE the sum of the terms that contain a
    moved atom for the new species minus for the old ones (``np.longdouble``; float64 with ``extended=False``), M the sum of
    those terms' magnitudes over both assignments.  A move that changes nothing has dE = M = 0 exactly."""
    so, dtype = _kind(extended)
    c1, c2, c3 = split_coefficients(ob, coefficients)
    fv = _FrameView(atoms)
    a = np.ascontiguousarray(i, dtype=np.int32).reshape(-1)
    b = _mc_second(mode, j_or_species)
    if len(a) != len(b):
        raise ValueError("mc_delta_x: as many first atoms as second atoms or species")
    dE, M = np.zeros(len(a), dtype), np.zeros(len(a))
    rc = so.uf3o_mc_delta_x(C.byref(ob.spec), C.byref(fv.c), _ptr(c1), _ptr(c2), _ptr(c3), C.c_int64(len(a)), _ptr(a), _ptr(b),
                            C.c_int(MC_MODES[mode]), _ptr(dE), _ptr(M))
    if rc:
        raise RuntimeError(f"uf3o_mc_delta_x rc={rc}")
    return dE, M


def mc_terms_x(ob, atoms, coefficients, i, j_or_species, mode, extended=False):
    """One move with the terms it is made of: ``(dE, M, terms)``, ``terms`` [n, len(MC_TERM_FIELDS)] float64 in the order of the
    oracle's term loop, the pass over the old species (``pass`` 0) before the pass over the new ones (1).  ``kind``: 1 one-body,
    2 directed pair term, 3 triplet; ``centre``, ``p1``, ``p2``: the parent atoms (-1: none); ``distance``: the pair distance, or
    r_jk of a triplet; ``legs_exchanged`` / ``leg_fp32``: the triplet's value with its l and m leg lengths exchanged / with its l
    leg length rounded through fp32 (for planted defects); ``r_ij``, ``r_ik``: a triplet's centre legs in the order (l, m).  dE = sum(value | pass 1) - sum(value | pass 0) up to summation order."""
    so, dtype = _kind(extended)
    c1, c2, c3 = split_coefficients(ob, coefficients)
    fv = _FrameView(atoms)
    second = int(_mc_second(mode, [j_or_species])[0])
    dE, M, n = np.zeros(1, dtype), np.zeros(1), np.zeros(1, dtype=np.int64)
    cap = 0
    while True:
        terms = np.zeros((max(cap, 1), len(MC_TERM_FIELDS)))
        rc = so.uf3o_mc_terms_x(C.byref(ob.spec), C.byref(fv.c), _ptr(c1), _ptr(c2), _ptr(c3), C.c_int(int(i)), C.c_int(second),
                                C.c_int(MC_MODES[mode]), _ptr(dE), _ptr(M), _ptr(terms), C.c_int64(len(terms)), _ptr(n))
        if rc:
            raise RuntimeError(f"uf3o_mc_terms_x rc={rc}")
        if int(n[0]) <= len(terms):
            return dE[0], M[0], terms[:int(n[0])].copy()
        cap = int(n[0])


def featurize(ob, atoms, energy=True, forces=True, indices=False):
    """
    Feature rows of one frame, reference column order without the ``y`` column.

    Returns dict(xe [F] | None, xf [N,3,F] | None) and, with ``indices=True``,
    ``pairs`` {pair: (n,2) int64 (i, j)} in np.where order, ``n3`` (n,2) int64
    (identify_ij, square=False) and ``supercell`` info.
    """
    fv = _FrameView(atoms)
    n = fv.c.n_atoms
    F = ob.n_feat
    xe = np.zeros(F) if energy else None
    xf = np.zeros((n, 3, F)) if forces else None
    out = {}
    pair_cnt = pair_ij = n3_cnt = n3_ij = sc_info = None
    cap2 = cap3 = 0
    if indices:
        sc_info = np.zeros(8, dtype=np.int64)
        pair_cnt = np.zeros(max(1, ob.spec.n_pairs), dtype=np.int64)
        n3_cnt = np.zeros(1, dtype=np.int64)
        rc = lib().uf3o_featurize(C.byref(ob.spec), C.byref(fv.c), None, None,
                                  _ptr(pair_cnt), None, C.c_int64(0),
                                  _ptr(n3_cnt), None, C.c_int64(0), _ptr(sc_info))
        if rc:
            raise RuntimeError(f"uf3o_featurize rc={rc}")
        cap2 = int(pair_cnt.max()) if len(pair_cnt) else 0
        cap3 = int(n3_cnt[0])
        pair_ij = np.zeros((max(1, ob.spec.n_pairs), max(1, cap2), 2), dtype=np.int64)
        n3_ij = np.zeros((max(1, cap3), 2), dtype=np.int64)
    rc = lib().uf3o_featurize(C.byref(ob.spec), C.byref(fv.c), _ptr(xe), _ptr(xf),
                              _ptr(pair_cnt), _ptr(pair_ij), C.c_int64(cap2),
                              _ptr(n3_cnt), _ptr(n3_ij), C.c_int64(cap3), _ptr(sc_info))
    if rc:
        raise RuntimeError(f"uf3o_featurize rc={rc}")
    out["xe"], out["xf"] = xe, xf
    if indices:
        out["pairs"] = {p: pair_ij[k, :pair_cnt[k]].copy() for k, p in enumerate(ob.pairs)}
        out["n3"] = n3_ij[:cap3].copy()
        out["supercell"] = dict(n_img=int(sc_info[0]), m=int(sc_info[1]),
                                factors=sc_info[2:5].tolist(), counts=sc_info[5:8].tolist())
    return out


def supercell(atoms, r_cut):
    fv = _FrameView(atoms)
    m = lib().uf3o_supercell(C.byref(fv.c), C.c_double(r_cut), None, None, None)
    pos = np.zeros((m, 3))
    z = np.zeros(m, dtype=np.int32)
    n_img = m // max(1, fv.c.n_atoms)
    shift = np.zeros((max(1, n_img), 3), dtype=np.int32)
    lib().uf3o_supercell(C.byref(fv.c), C.c_double(r_cut), _ptr(pos), _ptr(z), _ptr(shift))
    return pos, z, shift


def split_coefficients(ob, coefficients):
    """Flat model coefficients -> (c1, c2 concatenated, c3 concatenated full grids)."""
    basis = ob.basis
    coefficients = np.asarray(coefficients, dtype=np.float64)
    sizes, offsets = basis.get_interaction_partitions()
    n_el = len(basis.chemical_system.element_list)
    c1 = np.ascontiguousarray(coefficients[:n_el])
    c2 = [coefficients[offsets[p]:offsets[p] + sizes[p]] for p in ob.pairs]
    c3 = [basis.decompress_3B(coefficients[offsets[t]:offsets[t] + sizes[t]], t).ravel()
          for t in ob.trios]
    return (c1, np.ascontiguousarray(np.concatenate(c2)) if c2 else np.zeros(0),
            np.ascontiguousarray(np.concatenate(c3)) if c3 else np.zeros(0))


def evaluate(ob, atoms, coefficients, forces=True, virial=False):
    """Energy (and forces) of a model, calculator.py:156-343 restated.  With ``virial=True`` also the
    strain derivative dE/d(strain) [6] (eV, Voigt xx, yy, zz, yz, xz, xy): returns (e, f, v)."""
    c1, c2, c3 = split_coefficients(ob, coefficients)
    fv = _FrameView(atoms)
    e = C.c_double(0.0)
    f = np.zeros((fv.c.n_atoms, 3)) if forces else None
    if virial:
        v = np.zeros(6)
        rc = lib().uf3o_eval_virial(C.byref(ob.spec), C.byref(fv.c), _ptr(c1), _ptr(c2), _ptr(c3),
                                    C.byref(e), _ptr(f), _ptr(v))
        if rc:
            raise RuntimeError(f"uf3o_eval_virial rc={rc}")
        return e.value, f, v
    rc = lib().uf3o_eval(C.byref(ob.spec), C.byref(fv.c), _ptr(c1), _ptr(c2), _ptr(c3),
                         C.byref(e), _ptr(f))
    if rc:
        raise RuntimeError(f"uf3o_eval rc={rc}")
    return e.value, f


# ---------------------------------------------------------------------------
# NumPy restatement of the weighted normal-equation fit
# (uf3/regression/least_squares.py:274-353, 248-272, 716-771, 817-890, 1147-1169)
# ---------------------------------------------------------------------------
def fit(basis, regularizer, x_e, y_e, x_f=None, y_f=None, weight=0.5):
    n_feats = int(np.sum(basis.get_feature_partition_sizes()))
    col_idx, frozen_c = np.asarray(basis.col_idx, dtype=int), np.asarray(basis.frozen_c, float)
    mask = np.setdiff1d(np.arange(n_feats), col_idx)

    def freeze(x, y):
        return x[:, mask], y - x[:, col_idx] @ frozen_c

    x_e, y_e0 = np.asarray(x_e, float), np.asarray(y_e, float)
    xe, ye = freeze(x_e, y_e0)
    g, o = xe.T @ xe, xe.T @ ye
    parts = dict(gram_e=g.copy(), ord_e=o.copy())
    if x_f is not None:
        x_f, y_f0 = np.asarray(x_f, float), np.asarray(y_f, float)
        se, sf = np.std(y_e0), np.std(y_f0)
        if se == 0:
            we, wf = 1.0, 1 / np.sqrt(len(y_f0))
        else:
            we, wf = 1 / np.sqrt(len(y_e0)) / se, 1 / np.sqrt(len(y_f0)) / sf
        xf, yf = freeze(x_f, y_f0)
        gf, of = xf.T @ xf, xf.T @ yf
        parts.update(gram_f=gf.copy(), ord_f=of.copy(), energy_weight=we, force_weight=wf)
        g = weight * we ** 2 * g + (1 - weight) * wf ** 2 * gf
        o = weight * we ** 2 * o + (1 - weight) * wf ** 2 * of
    cov = np.zeros(n_feats, dtype=bool)
    cov[mask] = np.sum(g, axis=0) != 0
    r = np.asarray(regularizer, float)[:, mask]
    sol = np.linalg.solve(g + r.T @ r, o)
    full = np.zeros(n_feats)
    full[mask] = sol
    full[col_idx] = frozen_c
    parts.update(gram=g, ordinate=o, coefficients=full, data_coverage=cov)
    return parts
