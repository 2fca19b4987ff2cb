"""
``NudgedElasticBand``: nudged elastic bands on the device (``uf3_neb_*`` in ``libuf3hip.so``) -- migration barriers from a fitted
potential.  A band is a list of M >= 3 ``Atoms`` of equal atom count, species, cell and pbc; the first and the last are end
points and never move.  Positions, forces and every band's optimiser state stay in HBM; each step is one evaluator call over all
images of all bands (``UFCalculator``'s model, its MD route with a neighbour-list skin) and four small kernels.

The tangent is the improved tangent of Henkelman & Jonsson (2000); an ordinary image feels the true force perpendicular to the
tangent and the spring force ``k (|R_{i+1} - R_i| - |R_i - R_{i-1}|)`` along it; with ``climb`` the interior image of highest
energy at each evaluation feels the true force with its tangent component reversed and no spring.  Differences between
neighbouring images are taken as stored (positions are kept unwrapped, there is no minimum-image step): ``interpolate`` builds
bands for which that is right.  One FIRE (``Relaxation``'s constants and rules; ``maxstep`` bounds the norm of the band's whole
step) runs per band over all its interior images, as ASE optimises a band; a band has converged when every atom of every interior
image has |g_i| < ``fmax``.  A non-finite energy or force anywhere in a band, or a vanishing tangent, freezes that band alone with
status ``"nonfinite"``.

    images = neb.interpolate(initial, final, 7)
    with NudgedElasticBand(calc, images) as band:
        band.run(500, fmax=0.05)
        out = band.run(1500, fmax=0.05, climb=True)      # out["barrier"], out["energies"], out["climbing_image"] per band

``run`` may be called again: the FIRE state carries over, and ``run(a); run(b)`` follows ``run(a + b)``.  A band that converged
is tested again by the next run, whose ``fmax`` and ``climb`` may differ, and moves only if it fails that test.

``interpolate`` builds a band by linear interpolation of the positions, which drives atoms through each other on any path that
turns (an exchange, a dumbbell rotation, a ring).  ``idpp_interpolate`` relaxes that band on the image dependent pair potential
(``IDPP``; Smidstrup et al., J. Chem. Phys. 140, 214106; what ASE calls ``idpp_interpolate``), which needs no model, on the device
(``uf3_idpp_create``, ``uf3_amd/csrc/uf3_idpp.h``):

    images, info = neb.idpp_interpolate(initial, final, 7)

``CellNudgedElasticBand`` is the band whose images differ in cell (solid-state NEB: solid-solid transformations, ideal shear,
any path whose saddle wants another cell than its ends; ``uf3_ssneb_create``, the cell instances of ``uf3_amd/csrc/uf3_neb.h``).  It works in
``Relaxation(relax_cell=True)``'s generalised coordinates: with C0 the cell of a band's first image, image i has
D_i = C0^-1 C_i, q_i = x_i D_i^-1 and the vector u_i = (q_i, Y_i = kappa D_i) of 3 N + 9 numbers, kappa the band's
``cell_factor`` (default N, the relaxer's; Sheppard et al.'s Jacobian is volume^(1/3) N^(1/6)); its true force is
(F D_i^T, -D_i^-T W_i / kappa), W the strain derivative.  Tangents, springs, the climbing image and the one FIRE per band are the
rules above on these longer vectors, differences as stored; a band has converged when every atom row and every cell row of g
of every interior image is shorter than ``fmax``.  Every axis must be periodic, ``fixed`` is not supported, end images and their
cells never move.  Not done here: minimum-image tangents, IDPP on changing cells, an external pressure.

    final = neb.remove_cell_rotation(initial, final)                      # no rigid rotation along the band
    images = neb.interpolate(initial, final, 7, interpolate_cell=True)
    with CellNudgedElasticBand(calc, images) as band:
        out = band.run(1500, fmax=0.05, climb=True)
        cells = band.get_cells()
"""
import ctypes as C
import os
import warnings

import numpy as np

from uf3_amd import _lib
from uf3_amd.forcefield._driver import Driver, check_int, check_mask, check_real
from uf3_amd.forcefield.relax import STATUS

WHO = "NudgedElasticBand"


def _axes(cell, pbc):
    """The cell with the rows of its non-periodic axes replaced by unit vectors orthogonal to the rows already there, so that it
    can be inverted: the fraction along a non-periodic axis is taken along that direction, not along the stored cell row (which
    may be zero), and is never wrapped."""
    full = np.array(cell, dtype=float).reshape(3, 3)
    full[~pbc] = 0.0
    for k in np.flatnonzero(~pbc):
        full[k] = np.linalg.svd(full)[2][-1]             # (row k is zero: the last right singular vector spans the gap)
    return full


def _singular(cell):
    """True for a cell without volume to rounding (against the product of its row lengths), as ``uf3_ssneb_create`` tests it."""
    return not abs(np.linalg.det(cell)) > 1e-12 * np.prod(np.sqrt((cell * cell).sum(1)))


def interpolate(initial, final, n_images, mic=True, interpolate_cell=False):
    """``n_images`` frames from ``initial`` to ``final``, end points included, by linear interpolation of the positions.  With
    ``mic`` the displacement ``final - initial`` is wrapped to the minimum image along the periodic axes once, and the last
    image is ``initial + d``, unwrapped: neighbouring images then differ by d / (n_images - 1) as stored.

    ``interpolate_cell``: the end points may differ in cell (all axes periodic).  The cells are interpolated linearly and the
    positions in fractional coordinates, each image's taken in its own cell; with ``mic`` the fractional displacement is wrapped
    once.  Neighbouring images then differ by equal steps in the scaled coordinates ``CellNudgedElasticBand`` works in."""
    from uf3_amd.data.atoms import Atoms
    n_images = check_int(WHO, "n_images", n_images, 2)
    if len(initial) != len(final):
        raise ValueError(f"interpolate: the end points hold {len(initial)} and {len(final)} atoms")
    z = np.asarray(initial.get_atomic_numbers())
    if not np.array_equal(z, np.asarray(final.get_atomic_numbers())):
        raise ValueError("interpolate: the end points differ in species")
    if not isinstance(interpolate_cell, (bool, np.bool_)):
        raise ValueError(f"interpolate: interpolate_cell must be True or False, got {interpolate_cell!r}")
    cell = np.array(initial.get_cell(), dtype=float).reshape(3, 3)
    cell1 = np.array(final.get_cell(), dtype=float).reshape(3, 3)
    if not interpolate_cell and not np.array_equal(cell, cell1):
        raise ValueError("interpolate: the end points differ in cell")
    pbc = np.asarray(initial.get_pbc(), dtype=bool).reshape(3)
    if not np.array_equal(pbc, np.asarray(final.get_pbc(), dtype=bool).reshape(3)):
        raise ValueError("interpolate: the end points differ in pbc")
    if interpolate_cell:
        if not pbc.all():
            raise ValueError("interpolate: interpolate_cell needs end points periodic along all three axes")
        if not (np.all(np.isfinite(cell)) and np.all(np.isfinite(cell1))) or _singular(cell) or _singular(cell1):
            raise ValueError("interpolate: interpolate_cell needs end points with finite cells that are not singular")
        s0 = np.asarray(initial.get_positions(), dtype=float) @ np.linalg.inv(cell)
        ds = np.asarray(final.get_positions(), dtype=float) @ np.linalg.inv(cell1) - s0
        if mic:
            ds -= np.round(ds)
        out = []
        for k in range(n_images):
            t = k / (n_images - 1)
            ck = cell + (cell1 - cell) * t
            out.append(Atoms(numbers=z, positions=(s0 + ds * t) @ ck, cell=ck, pbc=pbc))
        return out
    x0 = np.asarray(initial.get_positions(), dtype=float)
    d = np.asarray(final.get_positions(), dtype=float) - x0
    if mic and pbc.any():
        full = _axes(cell, pbc)
        frac = d @ np.linalg.inv(full)
        frac[:, pbc] -= np.round(frac[:, pbc])
        d = frac @ full
    return [Atoms(numbers=z, positions=x0 + d * (k / (n_images - 1)), cell=cell, pbc=pbc) for k in range(n_images)]


def remove_cell_rotation(initial, final):
    """``final`` turned rigidly (cell and positions; the energy does not change) so that C0^-1 C_final, C0 the cell of
    ``initial``, is symmetric positive definite: the polar decomposition of the deformation between the two cells.  A band
    between ``initial`` and the result holds no rigid rotation, which no force would ever remove.  Host only."""
    from uf3_amd.data.atoms import Atoms
    c0 = np.array(initial.get_cell(), dtype=float).reshape(3, 3)
    c1 = np.array(final.get_cell(), dtype=float).reshape(3, 3)
    if not (np.all(np.isfinite(c0)) and np.all(np.isfinite(c1))) or _singular(c0) or _singular(c1):
        raise ValueError("remove_cell_rotation: both cells must be finite and not singular")
    d = np.linalg.inv(c0) @ c1
    if np.linalg.det(d) < 0:
        raise ValueError("remove_cell_rotation: the two cells differ in handedness")
    u, _, vt = np.linalg.svd(d)
    rot = u @ vt                                         # d = p rot with p symmetric positive definite; d rot^T = p
    return Atoms(numbers=final.get_atomic_numbers(), positions=np.asarray(final.get_positions(), dtype=float) @ rot.T,
                 cell=c1 @ rot.T, pbc=final.get_pbc())


def _bands_of(bands, who=WHO):
    if isinstance(bands, (list, tuple)) and bands and isinstance(bands[0], (list, tuple)):
        return False, [list(b) for b in bands]
    if not isinstance(bands, (list, tuple)):
        raise ValueError(f"{who}: bands must be a list of Atoms or a list of such lists")
    return True, [list(bands)]


def _check_band(k, band, who=WHO, cells_differ=False):
    if len(band) < 3:
        raise ValueError(f"{who}: band {k} has {len(band)} images; a band needs at least 3")
    a0 = band[0]
    if len(a0) < 1:
        raise ValueError(f"{who}: band {k} has no atoms")
    z0 = np.asarray(a0.get_atomic_numbers())
    c0 = np.array(a0.get_cell(), dtype=float).reshape(3, 3)
    p0 = np.asarray(a0.get_pbc(), dtype=bool).reshape(3)
    for j, a in enumerate(band[1:], 1):
        if len(a) != len(a0):
            raise ValueError(f"{who}: band {k}, image {j}: atom count differs from image 0")
        if not np.array_equal(np.asarray(a.get_atomic_numbers()), z0):
            raise ValueError(f"{who}: band {k}, image {j}: species differ from image 0")
        if not cells_differ and not np.array_equal(np.array(a.get_cell(), dtype=float).reshape(3, 3), c0):
            raise ValueError(f"{who}: band {k}, image {j}: cell differs from image 0")
        if not np.array_equal(np.asarray(a.get_pbc(), dtype=bool).reshape(3), p0):
            raise ValueError(f"{who}: band {k}, image {j}: pbc differs from image 0")
        if np.array_equal(np.asarray(a.get_positions(), dtype=float), np.asarray(band[j - 1].get_positions(), dtype=float)):
            raise ValueError(f"{who}: band {k}, image {j}: positions identical to image {j - 1}")


class _Bands(Driver):
    """What ``NudgedElasticBand`` and ``IDPP`` share: the checks of the bands, the state getters and the run on a ``uf3_neb``
    handle."""
    KIND = "neb"
    CELLS_DIFFER = False

    def _setup(self, bands, spring, fixed):
        """Every check of ``bands``, ``spring`` and ``fixed``, and ``self._batch``: nothing here touches the device."""
        who = self.WHO
        self._single, self.bands = _bands_of(bands, who)
        for k, band in enumerate(self.bands):
            _check_band(k, band, who, self.CELLS_DIFFER)
        nb = len(self.bands)
        sp = np.asarray(spring, dtype=float)
        if sp.ndim == 0:
            sp = np.full(nb, float(sp))
        if sp.shape != (nb,):
            raise ValueError(f"{who}: spring must be a scalar or hold one value per band ({nb}), got shape {sp.shape}")
        if not np.all(np.isfinite(sp)) or np.any(sp <= 0.0):
            raise ValueError(f"{who}: spring must be positive and finite")
        self.spring = np.ascontiguousarray(sp)
        self.frames = [a for band in self.bands for a in band]
        self.band_first = np.ascontiguousarray(np.cumsum([0] + [len(b) for b in self.bands]), dtype=np.int32)
        self._batch = _lib.FrameBatch(self.frames)
        if not np.all(np.isfinite(self._batch.pos)):
            raise ValueError(f"{who}: positions must be finite")
        if not np.all(np.isfinite(self._batch.cells)):
            raise ValueError(f"{who}: cells must be finite")
        self.fixed = check_mask(who, "fixed", fixed, self._batch.n_atoms)
        if self.fixed is not None:
            m = self.fixed
            off = self._batch.offsets
            for k in range(nb):
                f0, f1 = self.band_first[k], self.band_first[k + 1]
                for f in range(f0 + 1, f1):
                    if not np.array_equal(m[off[f]:off[f + 1]], m[off[f0]:off[f0 + 1]]):
                        raise ValueError(f"{who}: band {k}, image {f - f0}: fixed mask differs from image 0")

    # ---- state ------------------------------------------------------------------------------------------------------------
    def _state(self, *which):
        nf, n, nb = self._batch.n_frames, self._batch.n_atoms, len(self.bands)
        shapes = dict(pos=((n, 3), float), forces=((n, 3), float), neb_forces=((n, 3), float), energies=((nf,), float),
                      status=((nb,), np.int32), steps=((nb,), np.int64), criterion=((nb,), float), climbing=((nb,), np.int32))
        return self._fetch(shapes, which)

    def _per_band(self, x):
        return [x[self.band_first[k]:self.band_first[k + 1]].copy() for k in range(len(self.bands))]

    def get_positions(self):
        """[N, 3] Angstrom, the images of all bands concatenated, unwrapped."""
        return self._state("pos")["pos"]

    def get_forces(self):
        """[N, 3]: the true forces at the current positions (eV / Angstrom; ``IDPP``: F = -dS/dx, 1 / Angstrom^3)."""
        return self._state("forces")["forces"]

    def get_neb_forces(self):
        """[N, 3], the forces' unit: the NEB forces g at the current positions (0 on end points and fixed atoms; climbing as
        in the last run)."""
        return self._state("neb_forces")["neb_forces"]

    def get_potential_energies(self):
        """One array [M] per band at the current positions (eV; ``IDPP``: S, 1 / Angstrom^2)."""
        return self._per_band(self._state("energies")["energies"])

    def get_images(self):
        """The bands at the current positions: a list of lists of ``Atoms`` (one list when one band was given)."""
        from uf3_amd.data.atoms import Atoms
        x = self._state("pos")["pos"]
        off = self._batch.offsets
        flat = [Atoms(numbers=a.get_atomic_numbers(), positions=x[off[k]:off[k + 1]], cell=a.get_cell(), pbc=a.get_pbc())
                for k, a in enumerate(self.frames)]
        out = [flat[self.band_first[k]:self.band_first[k + 1]] for k in range(len(self.bands))]
        return out[0] if self._single else out

    # ---- optimisation -----------------------------------------------------------------------------------------------------
    def _run(self, max_steps, fmax, climb, dt, dt_max, maxstep, check_every, record_every, skin):
        who = self.WHO
        max_steps = check_int(who, "max_steps", max_steps)
        fmax = check_real(who, "fmax", fmax, strict=True)
        if not isinstance(climb, (bool, np.bool_)):
            raise ValueError(f"{who}: climb must be True or False, got {climb!r}")
        dt = check_real(who, "dt", dt, strict=True)
        dt_max = check_real(who, "dt_max", dt_max, strict=True)
        maxstep = check_real(who, "maxstep", maxstep, strict=True)
        check_every = check_int(who, "check_every", check_every, 1)
        record_every = check_int(who, "record_every", record_every)
        skin = check_real(who, "skin", skin, hi=4.0)
        handle = self._live()
        nf, nb = self._batch.n_frames, len(self.bands)
        n_rec = max_steps // record_every + 1 if record_every else 0
        raw = np.zeros((n_rec, nf + 2 * nb))
        self.ctx.check(self.ctx.lib.uf3_neb_run(handle, max_steps, fmax, dt, dt_max, maxstep, skin, int(climb), check_every,
                                                record_every, _lib._p(raw) if n_rec else None))
        s = self._state("status", "steps", "criterion", "climbing", "energies")   # (the last evaluation's: nothing has moved since)
        energies = self._per_band(s["energies"])
        out = dict(status=[STATUS[int(x)] for x in s["status"]], converged=s["status"] == 1, steps=s["steps"],
                   criterion=s["criterion"], energies=energies, barrier=np.array([e.max() - e[0] for e in energies]),
                   reverse_barrier=np.array([e.max() - e[-1] for e in energies]), climbing_image=s["climbing"])
        if n_rec:
            tail = raw[:, nf:].reshape(n_rec, nb, 2)
            out["records"] = dict(iteration=record_every * np.arange(n_rec, dtype=np.int64), energies=raw[:, :nf].copy(),
                                  criterion=tail[..., 0].copy(), climbing_image=tail[..., 1].astype(np.int32))
        return out


class NudgedElasticBand(_Bands):
    """Batched nudged-elastic-band relaxation of one or more bands on the device (module text above).

    Atoms outside the cell: positions are kept unwrapped and go to the evaluator as they are, and the evaluator takes the
    reference's finite image range around the positions as given (``include/uf3_hip.h``, above ``uf3_md_create``; DESIGN.md
    section 7).  An atom that leaves its cell along a band or while it relaxes loses the interactions that range no longer reaches from where it
    is: energies and forces are then ``evaluate_frames``' of the unwrapped positions, not the wrapped crystal's.  Start from
    wrapped frames, and describe a path that crosses a cell face in a cell (or with an origin) in which every image stays inside."""
    WHO = WHO

    def __init__(self, calc, bands, spring=0.1, fixed=None, skin=0.5, device=None):
        """``bands``: one band (a list of ``Atoms``) or a list of bands.  ``spring`` (eV / Angstrom^2): a scalar or one value
        per band.  ``fixed``: boolean mask [sum N] over the concatenated images of all bands (ASE's FixAtoms), the same in
        every image of a band: those atoms feel no force, never move and do not enter tangents or spring lengths.  ``skin``
        (Angstrom): the evaluator's neighbour-list skin during runs."""
        # every argument is checked before the device is touched
        self.skin = check_real(WHO, "skin", skin, hi=4.0)
        self._setup(bands, spring, fixed)
        self.calculator = calc
        self._create(calc, device, [_lib._p(self._batch.pos), _lib._p(self._batch.z), _lib._p(self.fixed)],
                     [len(self.bands), _lib._p(self.band_first), _lib._p(self.spring)])

    def run(self, max_steps, fmax=0.05, climb=False, dt=0.1, dt_max=1.0, maxstep=0.2, check_every=10, record_every=0):
        """Up to ``max_steps`` FIRE steps of every band still running (evaluations 0 .. max_steps).  Returns per band:
        ``status`` ("running" | "converged" | "nonfinite"), ``converged`` (bool), ``steps`` (moves made in all runs so far),
        ``criterion`` (the largest per-atom |g|), ``energies`` (a list of arrays [M]), ``barrier`` (max E - E_0),
        ``reverse_barrier`` (max E - E_{M-1}) and ``climbing_image`` (index within the band, -1: none) at the last evaluation;
        with ``record_every`` > 0 also ``records``: ``iteration`` [n_rec], ``energies`` [n_rec, n_frames], ``criterion`` and
        ``climbing_image`` [n_rec, n_bands] of evaluations 0, record_every, ... (after every band stopped, the final values
        repeat)."""
        return self._run(max_steps, fmax, climb, dt, dt_max, maxstep, check_every, record_every, self.skin)


class CellNudgedElasticBand(_Bands):
    """Batched nudged elastic bands whose images differ in cell, on the device (module text above; ``uf3_ssneb_create``).
    What ``NudgedElasticBand`` says about atoms outside the cell holds here too."""
    WHO = "CellNudgedElasticBand"
    CELLS_DIFFER = True

    def __init__(self, calc, bands, spring=0.1, cell_factor=None, device=None):
        """``bands``: one band (a list of ``Atoms``; ``interpolate(..., interpolate_cell=True)`` makes one) or a list of bands,
        every frame periodic along all three axes with a cell that is not singular.  ``spring`` (eV / Angstrom^2): a scalar or
        one value per band.  ``cell_factor`` (kappa): None (each band's atom count per image), a scalar or one value per band,
        positive and finite."""
        # every argument is checked before the device is touched
        who = self.WHO
        if device is not None:
            device = check_int(who, "device", device)
        self._setup(bands, spring, None)
        nb = len(self.bands)
        for k, band in enumerate(self.bands):
            for j, a in enumerate(band):
                if not np.all(np.asarray(a.get_pbc(), dtype=bool).reshape(3)):
                    raise ValueError(f"{who}: band {k}, image {j}: a cell band needs frames periodic along all three axes")
                if _singular(np.array(a.get_cell(), dtype=float).reshape(3, 3)):
                    raise ValueError(f"{who}: band {k}, image {j}: the cell is singular")
        if cell_factor is None:
            cf = np.array([float(len(b[0])) for b in self.bands])
        else:
            try:
                cf = np.asarray(cell_factor, dtype=float)
            except (TypeError, ValueError):
                raise ValueError(f"{who}: cell_factor must be None, a number or one number per band") from None
            if cf.ndim == 0:
                cf = np.full(nb, float(cf))
            if cf.shape != (nb,):
                raise ValueError(f"{who}: cell_factor must be a scalar or hold one value per band ({nb}), got shape {cf.shape}")
            if not np.all(np.isfinite(cf)) or np.any(cf <= 0.0):
                raise ValueError(f"{who}: cell_factor must be positive and finite")
        self.cell_factor = np.ascontiguousarray(cf)
        self.calculator = calc
        self.ctx = _lib.get_context(calc.device if device is None else device)
        self._dbasis = _lib.device_basis(calc.bspline_config, self.ctx)
        self._pid = os.getpid()
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.uf3_ssneb_create(self._dbasis.handle, C.byref(self._batch.struct), _lib._p(self._batch.pos),
                                                     _lib._p(self._batch.z), _lib._p(calc._c1), _lib._p(calc._c2),
                                                     _lib._p(calc._c3), nb, _lib._p(self.band_first), _lib._p(self.spring),
                                                     _lib._p(self.cell_factor), C.byref(h)))
        self.handle = h

    def run(self, max_steps, fmax=0.05, climb=False, dt=0.1, dt_max=1.0, maxstep=0.2, check_every=10, record_every=0):
        """``NudgedElasticBand.run`` (no skin: the cells change, every step builds its lists anew).  ``criterion``: the largest
        row norm of g over the atom rows (eV / Angstrom, in scaled coordinates) and the cell rows of every interior image;
        ``maxstep`` bounds the band's whole step over atoms and cells."""
        return self._run(max_steps, fmax, climb, dt, dt_max, maxstep, check_every, record_every, 0.0)

    def _cell_state(self, *which):
        nf = self._batch.n_frames
        shapes = dict(cells=(nf, 3, 3), virials=(nf, 6), cell_forces=(nf, 3, 3), neb_cell_forces=(nf, 3, 3))
        out = {k: np.empty(shapes[k]) for k in which}
        self.ctx.check(self.ctx.lib.uf3_neb_get_cell_state(self._live(), *[_lib._p(out[k]) if k in out else None for k in shapes]))
        return out

    def get_cells(self):
        """[n_frames, 3, 3] Angstrom: the current cell of every image of every band."""
        return self._cell_state("cells")["cells"]

    def get_virials(self):
        """[n_frames, 6]: dE/d(strain) (xx, yy, zz, yz, xz, xy; eV) at the current state."""
        return self._cell_state("virials")["virials"]

    def get_cell_forces(self):
        """[n_frames, 3, 3]: the true force on Y = kappa D of every image, -D^-T W / kappa.  (``get_forces``: F D^T.)"""
        return self._cell_state("cell_forces")["cell_forces"]

    def get_neb_cell_forces(self):
        """[n_frames, 3, 3]: the cell part of the NEB force g (0 on end points; climbing as in the last run)."""
        return self._cell_state("neb_cell_forces")["neb_cell_forces"]

    def get_images(self):
        """The bands at the current positions, each image with its own current cell."""
        from uf3_amd.data.atoms import Atoms
        x, cells = self._state("pos")["pos"], self.get_cells()
        off = self._batch.offsets
        flat = [Atoms(numbers=a.get_atomic_numbers(), positions=x[off[k]:off[k + 1]], cell=cells[k], pbc=a.get_pbc())
                for k, a in enumerate(self.frames)]
        out = [flat[self.band_first[k]:self.band_first[k + 1]] for k in range(len(self.bands))]
        return out[0] if self._single else out


class IDPP(_Bands):
    """Bands relaxed on the image dependent pair potential on the device (``uf3_idpp_create``): for image k of a band of M
    images, lambda = k / (M - 1), over all pairs with one image each,

        S = sum_{i<j} (t_ij - d_ij)^2 / d_ij^4,    t_ij = (1 - lambda) d_ij(first image) + lambda d_ij(last image),

    with d_ij the nearest-image distance (``include/uf3_hip.h`` above ``uf3_idpp_create``: exact for every cell whose nearest
    image lies within one cell of the rounded fractional difference; a pair at exactly half a cell is a kink of S).  The band
    mechanics are ``NudgedElasticBand``'s (improved tangent, springs, one FIRE per band, the same statuses) with S as the
    energy (1 / Angstrom^2) and F = -dS/dx as the force (1 / Angstrom^3); there is no climbing image, no neighbour list and no
    calculator.  Fixed atoms count in every sum and feel no force.  Two atoms of an image at one position make S non-finite:
    that band ends ``"nonfinite"``."""
    WHO = "IDPP"

    def __init__(self, bands, spring=0.1, fixed=None, device=None):
        """``bands``, ``fixed``: as on ``NudgedElasticBand``.  ``spring`` (1 / Angstrom^4): a scalar or one value per band."""
        # every argument is checked before the device is touched
        if device is not None:
            device = check_int(self.WHO, "device", device)
        self._setup(bands, spring, fixed)
        self.ctx = _lib.get_context(device)
        self._pid = os.getpid()
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.uf3_idpp_create(self.ctx.handle, C.byref(self._batch.struct), _lib._p(self._batch.pos),
                                                    _lib._p(self._batch.z), _lib._p(self.fixed), len(self.bands),
                                                    _lib._p(self.band_first), _lib._p(self.spring), C.byref(h)))
        self.handle = h

    def run(self, max_steps, fmax=0.1, dt=0.1, dt_max=1.0, maxstep=0.2, check_every=10, record_every=0):
        """``NudgedElasticBand.run`` without ``climb``: ``criterion`` and ``fmax`` in 1 / Angstrom^3, ``energies`` S per image;
        ``climbing_image`` is -1 throughout."""
        return self._run(max_steps, fmax, False, dt, dt_max, maxstep, check_every, record_every, 0.0)


def idpp_interpolate(initial, final, n_images, mic=True, fmax=0.1, max_steps=1000, **kw):
    """``interpolate(initial, final, n_images, mic)``, then that band relaxed by ``IDPP`` until every atom of every interior
    image has |g_i| < ``fmax`` (1 / Angstrom^3; 0.1 is ASE's default) or for ``max_steps`` steps.  ``initial`` and ``final`` may
    be lists of equal length: one band each, relaxed in one batch.  ``kw``: ``spring``, ``fixed``, ``device`` of ``IDPP`` and
    ``dt``, ``dt_max``, ``maxstep``, ``check_every`` of its ``run``.  Returns (images, info): the band (a list of bands for
    lists), unwrapped like ``interpolate``'s, and ``IDPP.run``'s result.  Warns (``RuntimeWarning``) for each band that did
    not converge."""
    who = "idpp_interpolate"
    many = isinstance(initial, (list, tuple))
    if many != isinstance(final, (list, tuple)):
        raise ValueError(f"{who}: initial and final must both be Atoms or both be lists")
    ini, fin = (list(initial), list(final)) if many else ([initial], [final])
    if len(ini) != len(fin) or not ini:
        raise ValueError(f"{who}: initial and final hold {len(ini)} and {len(fin)} frames")
    n_images = check_int(who, "n_images", n_images, 3)
    fmax = check_real(who, "fmax", fmax, strict=True)
    max_steps = check_int(who, "max_steps", max_steps)
    make = {k: kw.pop(k) for k in ("spring", "fixed", "device") if k in kw}
    run = {k: kw.pop(k) for k in ("dt", "dt_max", "maxstep", "check_every") if k in kw}
    if kw:
        raise ValueError(f"{who}: unknown arguments {sorted(kw)}")
    bands = [interpolate(a, b, n_images, mic=mic) for a, b in zip(ini, fin)]
    with IDPP(bands, **make) as band:
        info = band.run(max_steps, fmax=fmax, **run)
        images = band.get_images()
    for k, status in enumerate(info["status"]):
        if status != "converged":
            warnings.warn(f"{who}: band {k} did not converge ({status}): criterion {info['criterion'][k]:.3g} 1 / Angstrom^3 "
                          f"after {int(info['steps'][k])} steps", RuntimeWarning, stacklevel=2)
    return (images if many else images[0]), info
