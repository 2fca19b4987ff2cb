"""
``UFCalculator``: energy and forces of a fitted UF3 model on the MI355X.

Surface follows the reference's ``uf3/forcefield/calculator.py`` (:40-153, helpers
:490-573): ``UFCalculator(model)``, ASE's ``calculate(atoms, properties,
system_changes)`` protocol with ``results['energy'|'free_energy'|'forces'|'stress']``,
``get_potential_energy`` / ``get_forces``.  The evaluation is the featurizer's
traversal contracted with the coefficients on the fly (``uf3_eval`` in
``libuf3hip.so``): pair splines from the pair coefficient vectors, trio splines from
the decompressed L x M x N grids (``decompress_3B``), as the reference builds its
``ndsplines`` objects.  Stress is analytic (the strain derivative is accumulated in the same
pass, ``uf3_eval_virial``; the reference differentiates the energy numerically,
``calculator.py:399-404``).  ASE is optional: the class derives from ``ase``'s Calculator when
ASE is importable and is otherwise a duck-typed stand-alone.
"""
import ctypes as C

import os

import numpy as np

from uf3_amd import _lib

try:  # pragma: no cover - ASE is not installed on the build / GPU boxes
    from ase.calculators.calculator import Calculator as _Base, all_changes
except Exception:  # noqa: BLE001
    all_changes = ['positions', 'numbers', 'cell', 'pbc', 'initial_charges', 'initial_magmoms']

    class _Base:
        def __init__(self, **kwargs):
            self.results = {}
            self.atoms = None

        def calculate(self, atoms=None, properties=None, system_changes=all_changes):
            if atoms is not None:
                self.atoms = atoms.copy() if hasattr(atoms, "copy") else atoms

        def get_property(self, name, atoms=None, allow_calculation=True):
            self.calculate(atoms, [name], all_changes)
            return self.results[name]

        def get_potential_energy(self, atoms=None, force_consistent=False):
            return self.get_property('energy', atoms)

        def get_forces(self, atoms=None):
            return self.get_property('forces', atoms)

        def get_stress(self, atoms=None):
            return self.get_property('stress', atoms)


def coefficients_by_interaction(element_list, interactions_map, partition_sizes, coefficients):
    parts = np.array_split(coefficients, np.cumsum(partition_sizes)[:-1])
    n = len(element_list)
    solutions = {el: v for el, v in zip(element_list, parts[:n])}
    for idx, key in enumerate(list(interactions_map[2]) + list(interactions_map.get(3, []))):
        solutions[key] = parts[n + idx]
    return solutions


AUTO_MD_SKIN = 0.5        # Angstrom: the skin of ``md_skin="auto"``


class UFCalculator(_Base):
    implemented_properties = ['energy', 'forces', 'stress']

    def __init__(self, model, device=None, md_skin=None, **kwargs):
        """``md_skin`` (Angstrom): keep the device's neighbour lists between calls out to ``r_cut + md_skin`` and rebuild them
        only when an atom has moved more than ``md_skin / 2`` (``_lib.Context.md_skin``) -- what an MD or relaxation loop
        wants; 0 rebuilds everything on every call like the reference (``calculator.py:124-153``).  Default (``None``): the
        environment's ``UF3_MD_SKIN`` if set, else ``"auto"`` -- a skin of 0.5 Angstrom from the second consecutive call on
        the same single frame (atom count, cell, boundary conditions) on, nothing kept for one-off calls on changing structures.
        Results do not depend on the setting beyond rounding (1e-13), nor on when the lists were built."""
        super().__init__(**kwargs)
        self.bspline_config = model.bspline_config
        self.model = model
        self.device = device
        if md_skin is None:
            md_skin = os.environ.get("UF3_MD_SKIN", "auto")
        self.md_auto = isinstance(md_skin, str) and md_skin.strip().lower() == "auto"
        self.md_skin = AUTO_MD_SKIN if self.md_auto else float(md_skin)
        self._last_batch = None
        self._last_layout = None
        basis = self.bspline_config
        self.solutions = coefficients_by_interaction(basis.element_list, basis.interactions_map,
                                                     basis.partition_sizes, model.coefficients)
        self.pair_potentials = {p: np.asarray(self.solutions[p], dtype=float)
                                for p in basis.interactions_map[2]}
        self.trio_potentials = {}
        if basis.degree > 2:
            self.trio_potentials = {t: basis.decompress_3B(np.asarray(self.solutions[t], dtype=float), t)
                                    for t in basis.interactions_map[3]}
        self._c1 = np.ascontiguousarray([float(np.ravel(self.solutions[el])[0]) for el in basis.element_list])
        self._c2 = np.ascontiguousarray(np.concatenate([self.pair_potentials[p] for p in basis.interactions_map[2]]))
        self._c3 = (np.ascontiguousarray(np.concatenate([self.trio_potentials[t].ravel()
                                                         for t in basis.interactions_map[3]]))
                    if self.trio_potentials else np.zeros(1))
        self._pc = (_lib._addr(self._c1), _lib._addr(self._c2), _lib._addr(self._c3))     # (the arrays live as long as self)

    degree = property(lambda self: self.bspline_config.degree)
    element_list = property(lambda self: self.bspline_config.element_list)
    interactions_map = property(lambda self: self.bspline_config.interactions_map)
    r_min_map = property(lambda self: self.bspline_config.r_min_map)
    r_max_map = property(lambda self: self.bspline_config.r_max_map)
    r_cut = property(lambda self: self.bspline_config.r_cut)
    partition_sizes = property(lambda self: self.bspline_config.partition_sizes)
    coefficients = property(lambda self: self.model.coefficients)
    chemical_system = property(lambda self: self.bspline_config.chemical_system)

    def __repr__(self):
        return "\n".join(["UFCalculator:", repr(self.model)])

    def evaluate_frames(self, atoms_list, forces=True, virial=False):
        """Energies [n_frames], forces [sum N, 3] (and dE/d(strain) [n_frames, 6]) of a batch of frames."""
        ctx = _lib.get_context(self.device)
        db = _lib.device_basis(self.bspline_config, ctx)
        # (an MD loop hands over the same single frame again and again: its batch is kept and refreshed in place)
        batch = self._last_batch
        if len(atoms_list) != 1 or batch is None or not batch.refresh(atoms_list[0]):
            batch = _lib.FrameBatch(atoms_list)
            self._last_batch = batch if len(atoms_list) == 1 else None
        skin = self.md_skin
        if self.md_auto:        # lists are worth keeping once the same single frame comes back
            layout = (batch.n_atoms, batch.cells.tobytes(), batch.pbc.tobytes()) if batch.n_frames == 1 else None
            if layout is None or layout != self._last_layout:
                skin = 0.0
            self._last_layout = layout
        if getattr(ctx, "_md_skin", 0.0) != skin:
            ctx.md_skin(skin)
        e = np.empty(batch.n_frames)
        f = np.empty((batch.n_atoms, 3)) if forces else None
        addr = _lib._addr                     # (plain ints: the host side of an MD-step call is as long as its kernels)
        args = (db.handle, C.byref(batch.struct), addr(batch.pos), addr(batch.z), self._pc[0], self._pc[1], self._pc[2],
                addr(e), addr(f))
        if virial:
            v = np.empty((batch.n_frames, 6))
            rc = ctx.lib.uf3_eval_virial(*args, addr(v))
            if rc:
                ctx.check(rc)
            return e, f, batch.offsets, v
        rc = ctx.lib.uf3_eval(*args)
        if rc:
            ctx.check(rc)
        return e, f, batch.offsets

    def evaluate_atom_range(self, atoms, atom_begin, atom_end, forces=True, virial=False):
        """
        Share of atoms [atom_begin, atom_end) of one frame: (energy share, forces [N, 3] with the other
        atoms' rows zero, dE/d(strain) share [6] or None).  Shares over disjoint ranges covering the frame
        add up to ``evaluate_frames`` (``uf3_eval_atoms``; used by ``parallel.sharded_evaluate``).
        """
        ctx = _lib.get_context(self.device)
        db = _lib.device_basis(self.bspline_config, ctx)
        batch = _lib.FrameBatch([atoms])
        e = np.empty(1)
        f = np.empty((batch.n_atoms, 3)) if forces else None
        v = np.empty((1, 6)) if virial else None
        addr = _lib._addr
        ctx.check(ctx.lib.uf3_eval_atoms(db.handle, C.byref(batch.struct), addr(batch.pos), addr(batch.z), self._pc[0], self._pc[1],
                                         self._pc[2], int(atom_begin), int(atom_end), addr(e), addr(f), addr(v)))
        return float(e[0]), f, (v[0] if virial else None)

    def evaluate_centre_range(self, atoms, atom_begin, atom_end, forces=True, virial=False):
        """
        Share of the CENTRES [atom_begin, atom_end) of one frame: (energy share, forces [N, 3], dE/d(strain) share [6] or
        None).  Every triplet is evaluated once, at its centre inside the range, so the force array also carries what those
        triplets put on atoms outside it (the range's halo); all other rows are zero.  Shares over disjoint ranges covering
        the frame add up to ``evaluate_frames`` at a third of ``evaluate_atom_range``'s triplet work (``uf3_eval_centres``;
        what ``parallel.sharded_evaluate`` reduces).
        """
        ctx = _lib.get_context(self.device)
        skin = 0.0 if self.md_auto else self.md_skin            # (blocks of centres keep lists only when asked to)
        if getattr(ctx, "_md_skin", 0.0) != skin:
            ctx.md_skin(skin)                     # (with a skin the ranks' whole-frame lists live across steps)
        db = _lib.device_basis(self.bspline_config, ctx)
        batch = _lib.FrameBatch([atoms])
        e = np.empty(1)
        f = np.empty((batch.n_atoms, 3)) if forces else None
        v = np.empty((1, 6)) if virial else None
        addr = _lib._addr
        ctx.check(ctx.lib.uf3_eval_centres(db.handle, C.byref(batch.struct), addr(batch.pos), addr(batch.z), self._pc[0], self._pc[1],
                                           self._pc[2], int(atom_begin), int(atom_end), addr(e), addr(f), addr(v)))
        return float(e[0]), f, (v[0] if virial else None)

    def calculate(self, atoms=None, properties=None, system_changes=tuple(all_changes)):
        if properties is None:
            properties = self.implemented_properties
        _Base.calculate(self, atoms, properties, system_changes)
        want_f = 'forces' in properties
        if ('energy' in properties) or ('free_energy' in properties) or want_f:
            e, f, _ = self.evaluate_frames([atoms], forces=want_f)
            self.results['energy'] = float(e[0])
            self.results['free_energy'] = self.results['energy']
            if want_f:
                self.results['forces'] = f
        if 'stress' in properties:
            self.results['stress'] = self._get_stress(atoms)

    def _get_potential_energy(self, atoms=None, force_consistent=None):
        return float(self.evaluate_frames([atoms], forces=False)[0][0])

    def _get_forces(self, atoms=None):
        return self.evaluate_frames([atoms], forces=True)[1]

    def _get_stress(self, atoms=None, numerical=False, d=1e-6):
        """
        Stress in Voigt order (xx, yy, zz, yz, xz, xy), eV/A^3.  Default: analytic virial accumulated in
        the same neighbour traversal as the forces.  ``numerical=True`` reproduces the
        reference's route (central differences of the energy under strain, calculator.py:399-404), the 12
        strained copies going to the GPU as one batch.
        """
        cell = np.array(atoms.get_cell(), dtype=float).reshape(3, 3)
        vol = abs(np.linalg.det(cell))
        if not numerical:
            return self.evaluate_frames([atoms], forces=False, virial=True)[3][0] / vol
        pos = np.asarray(atoms.get_positions(), dtype=float)
        from uf3_amd.data.atoms import Atoms
        frames, pairs = [], [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
        for i, j in pairs:
            for sign in (+1, -1):
                eps = np.eye(3)
                if i == j:
                    eps[i, i] += sign * d
                else:
                    eps[i, j] += 0.5 * sign * d
                    eps[j, i] += 0.5 * sign * d
                frames.append(Atoms(numbers=atoms.get_atomic_numbers(), positions=pos @ eps, cell=cell @ eps,
                                    pbc=atoms.get_pbc()))
        e = self.evaluate_frames(frames, forces=False)[0]
        return np.array([(e[2 * k] - e[2 * k + 1]) / (2 * d * vol) for k in range(6)])

    # ---- per-atom resolution (uf3_site_terms / uf3_heat_flux) -------------------------------------------
    def site_terms(self, atoms_list, virials=True):
        """Site energies and site virials of a batch of frames: (U, W), lists with one array per frame, U[f] [N_f] (eV) and
        W[f] [N_f, 3, 3] (eV; ``None`` in place of the list when ``virials`` is false).  U_i is the evaluator's own partition of
        the energy (one-body term, the directed pair terms of i, the triplets with i as the centre): ``U[f].sum()`` is the
        frame's energy.  W_i[a][b] = sum over the terms of U_i and their neighbour images s of d_s[a] (dU_i/dr_s)[b], d_s from
        the centre to the image: the frame's sum, symmetrised, is ``evaluate_frames(..., virial=True)``'s dE/d(strain)."""
        ctx = _lib.get_context(self.device)
        db = _lib.device_basis(self.bspline_config, ctx)
        batch = _lib.FrameBatch(list(atoms_list))
        u = np.empty(batch.n_atoms)
        w = np.empty((batch.n_atoms, 3, 3)) if virials else None
        addr = _lib._addr
        ctx.check(ctx.lib.uf3_site_terms(db.handle, C.byref(batch.struct), addr(batch.pos), addr(batch.z), self._pc[0], self._pc[1],
                                         self._pc[2], addr(u), addr(w)))
        off = batch.offsets
        split = lambda a: [a[off[k]:off[k + 1]] for k in range(batch.n_frames)]     # noqa: E731
        return split(u), (split(w) if virials else None)

    def get_potential_energies(self, atoms=None):
        """ASE's per-atom energies [N] (eV): the site energies U_i of ``site_terms``; their sum is ``get_potential_energy``."""
        return self.site_terms([atoms], virials=False)[0][0]

    def _device_leverage(self, max_atoms_per_chunk):
        """The calculator's ``pipeline.DeviceLeverage``, made again when the chunk limit or the model's posterior changed."""
        from uf3_amd import pipeline
        from uf3_amd.representation import process
        lev = getattr(self, "_leverage", None)
        w = self.model.whitening()                                # (the ValueError, before anything touches the device)
        if lev is None or lev.max_atoms != int(max_atoms_per_chunk) or lev._w_host is not w:
            fz = process.BasisFeaturizer(self.bspline_config, device=self.device)
            lev = self._leverage = pipeline.DeviceLeverage(self.model, fz, max_atoms_per_chunk=max_atoms_per_chunk)
        return lev

    def get_leverages(self, atoms_or_list, forces=True, max_atoms_per_chunk=320000):
        """Leverages of one frame or a list of frames against the system this calculator's model was fitted on
        (``pipeline.DeviceLeverage``): ``dict(energy, force, offsets)``; for a single ``Atoms`` ``energy`` is a scalar and
        ``force`` has shape [N].  A model without a posterior (read from a file, no ``load_posterior``) raises ``ValueError``."""
        lev = self._device_leverage(max_atoms_per_chunk)
        single = not isinstance(atoms_or_list, (list, tuple))
        out = lev.frames([atoms_or_list] if single else list(atoms_or_list), forces=forces)
        if single:
            out["energy"] = float(out["energy"][0])
        return out

    def get_site_grades(self, atoms_or_list, max_atoms_per_chunk=320000):
        """Per-atom extrapolation grades of one frame or a list of frames against the system this calculator's model was
        fitted on (``pipeline.DeviceLeverage.sites``): ``dict(grade, frame_max, frame_argmax, offsets)``; for a single
        ``Atoms`` ``frame_max`` and ``frame_argmax`` are scalars.  The grades describe the wrapped frame, as ``site_terms``
        does.  A model without a posterior raises ``ValueError``."""
        lev = self._device_leverage(max_atoms_per_chunk)
        single = not isinstance(atoms_or_list, (list, tuple))
        out = lev.sites([atoms_or_list] if single else list(atoms_or_list))
        if single:
            out["frame_max"], out["frame_argmax"] = float(out["frame_max"][0]), int(out["frame_argmax"][0])
        return out

    def get_stresses(self, atoms=None):
        """Per-atom stresses [N, 6], eV/A^3, in ``get_stress``'s convention -- Voigt order (xx, yy, zz, yz, xz, xy) and ASE's
        sign (dE/d(strain) per volume: positive under tension) --, each atom given the volume V / N:
        ``sym(W_i) / (V / N)`` with the site virials of ``site_terms``, so that their MEAN over the atoms is ``get_stress``
        (no kinetic part).  The frame needs a cell with a volume."""
        cell = np.array(atoms.get_cell(), dtype=float).reshape(3, 3)
        vol = abs(np.linalg.det(cell))
        if not vol > 0:
            raise ValueError("get_stresses: the frame's cell has no volume")
        w = self.site_terms([atoms])[1][0]
        s = 0.5 * (w + w.transpose(0, 2, 1))
        voigt = np.stack([s[:, 0, 0], s[:, 1, 1], s[:, 2, 2], s[:, 1, 2], s[:, 0, 2], s[:, 0, 1]], axis=1)
        return voigt / (vol / len(w))

    def heat_flux(self, atoms_list, velocities, masses=None, site_energies=False):
        """The heat current of every frame, [n_frames, 2, 3] in eV A / fs: row 0 the convective part
        sum_i (1/2 m_i v_i^2 + U_i) v_i, row 1 the potential part -sum_i sum_terms sum_s d_s (dU_i/dr_s . v_s) (images carry
        their parent's velocity); J is their sum.  ``velocities`` [sum N, 3] in A / fs, frames concatenated; ``masses`` as
        ``md.resolve_masses`` takes them (amu).  With ``site_energies`` also the U_i [sum N].  A velocities array of another
        length, like a mass that is not positive and finite, is refused with the library's error (``UF3Error``, UF3_EINVAL)
        before anything is launched."""
        from .md import resolve_masses
        frames = list(atoms_list)
        ctx = _lib.get_context(self.device)
        db = _lib.device_basis(self.bspline_config, ctx)
        batch = _lib.FrameBatch(frames)
        v = np.ascontiguousarray(np.asarray(velocities, dtype=float))
        if v.shape != (batch.n_atoms, 3):
            raise _lib.UF3Error(1, f"uf3_heat_flux: velocities must be [{batch.n_atoms}, 3], got {list(v.shape)}")
        if masses is not None and not isinstance(masses, dict):
            m = np.ascontiguousarray(np.asarray(masses, dtype=float).reshape(-1))
            if m.shape != (batch.n_atoms,):
                raise _lib.UF3Error(1, f"uf3_heat_flux: {m.size} masses for {batch.n_atoms} atoms")
        else:
            m = resolve_masses(frames, masses)
        flux = np.empty((batch.n_frames, 2, 3))
        u = np.empty(batch.n_atoms) if site_energies else None
        addr = _lib._addr
        ctx.check(ctx.lib.uf3_heat_flux(db.handle, C.byref(batch.struct), addr(batch.pos), addr(v), addr(batch.z), addr(m),
                                        self._pc[0], self._pc[1], self._pc[2], addr(flux), addr(u)))
        return (flux, u) if site_energies else flux

    def relax_fmax(self, geom, fmax=0.05, relax_cell=True, verbose=False, timeout=60.0, max_steps=2000, dt=0.1):
        """
        Minimise the maximum force (reference: calculator.py:406-436, which drives ASE's BFGSLineSearch on an
        ExpCellFilter).  ASE is not a dependency here: the same objective -- atomic forces, plus for fully
        periodic frames with ``relax_cell`` the strain derivative (analytic virial) -- is minimised with FIRE
        (Bitzek et al., PRL 97, 170201).  Returns a relaxed copy; warns and returns the last iterate on timeout.
        """
        import time
        import warnings
        from uf3_amd.data.atoms import Atoms
        numbers = np.asarray(geom.get_atomic_numbers())
        pos = np.array(geom.get_positions(), dtype=float)
        cell0 = np.array(geom.get_cell(), dtype=float).reshape(3, 3)
        pbc = np.asarray(geom.get_pbc(), dtype=bool)
        with_cell = bool(relax_cell and np.all(pbc))
        n = len(numbers)
        # generalised coordinates: scaled positions * cell0 (so they are lengths) and, optionally, the deformation
        # gradient D (cell = cell0 @ D), weighted by n like ASE's cell filters
        frac = pos @ np.linalg.inv(cell0) if with_cell else None
        D = np.eye(3)
        x_vel = np.zeros((n + (3 if with_cell else 0), 3))
        alpha0, f_inc, f_dec, f_alpha, n_min, dt_max = 0.1, 1.1, 0.5, 0.99, 5, 10 * dt
        alpha, n_pos, t0 = alpha0, 0, time.time()

        def evaluate(pos_, cell_):
            frame = Atoms(numbers=numbers, positions=pos_, cell=cell_, pbc=pbc)
            if with_cell:
                e, f, _, v = self.evaluate_frames([frame], forces=True, virial=True)
                vv = v[0]
                sigma_v = np.array([[vv[0], vv[5], vv[4]], [vv[5], vv[1], vv[3]], [vv[4], vv[3], vv[2]]])   # dE/d(eps)
                return float(e[0]), f, sigma_v
            e, f, _ = self.evaluate_frames([frame], forces=True)
            return float(e[0]), f, None

        cell = cell0.copy()
        for step in range(max_steps):
            e, f, dE_deps = evaluate(pos, cell)
            if with_cell:
                # positions move with the cell: q = frac @ cell0, x = q @ D; dE/dq = -f @ D^T; dE/dD = D^-T dE/deps
                g_cell = -(np.linalg.inv(D).T @ dE_deps) / max(n, 1)
                force = np.vstack([f @ D.T, g_cell])
                crit = max(np.abs(f).max(), np.abs(dE_deps).max() / max(n, 1))
            else:
                force, crit = f, np.abs(f).max()
            if verbose:
                print(f"relax_fmax step {step}: E = {e:.8f}  max|F| = {np.abs(f).max():.5f}")
            if crit < fmax:
                break
            if (time.time() - t0) > timeout:
                warnings.warn("Relaxation timed out.", RuntimeWarning)
                break
            power = float(np.sum(force * x_vel))
            if power > 0:
                fn, vn = np.linalg.norm(force), np.linalg.norm(x_vel)
                x_vel = (1 - alpha) * x_vel + (alpha * vn / fn) * force if fn > 0 else x_vel
                n_pos += 1
                if n_pos > n_min:
                    dt, alpha = min(dt * f_inc, dt_max), alpha * f_alpha
            else:
                x_vel[:] = 0.0
                n_pos, dt, alpha = 0, dt * f_dec, alpha0
            x_vel = x_vel + dt * force
            step_x = dt * x_vel
            big = np.abs(step_x).max()
            if big > 0.2:                                   # trust radius (Angstrom / unit strain)
                step_x *= 0.2 / big
            if with_cell:
                q = frac @ cell0 + step_x[:n]
                frac = q @ np.linalg.inv(cell0)
                D = D + step_x[n:] / max(n, 1)
                cell = cell0 @ D
                pos = frac @ cell
            else:
                pos = pos + step_x
        return Atoms(numbers=numbers, positions=pos, cell=cell, pbc=pbc)

    def relax_frames(self, frames, fmax=0.05, relax_cell=False, max_steps=2000, **kw):
        """
        Relax a batch of frames at once on the device (``relax.Relaxation``: FIRE in ASE's formulation, every frame its own
        optimiser; with ``relax_cell`` fully periodic frames also relax their cell).  ``kw``: ``fixed``, ``skin``, ``device``
        (the object's) and ``dt``, ``dt_max``, ``maxstep``, ``check_every`` (``run``'s).  Returns (relaxed frames, info), info
        as ``Relaxation.run`` returns it; warns (RuntimeWarning) when a frame did not converge.  ``relax_fmax`` is the
        one-frame host loop it does not replace.
        """
        import warnings
        from .relax import Relaxation
        make = {k: kw.pop(k) for k in ("fixed", "skin", "device") if k in kw}
        with Relaxation(self, frames, relax_cell=relax_cell, **make) as rel:
            info = rel.run(max_steps, fmax=fmax, **kw)
            out = rel.get_atoms()
        if not np.all(info["converged"]):
            bad = [k for k, ok in enumerate(info["converged"]) if not ok]
            warnings.warn(f"relax_frames: {len(bad)} of {len(info['converged'])} frames did not converge (frames {bad[:10]}"
                          f"{', ...' if len(bad) > 10 else ''})", RuntimeWarning)
        return out, info

    def neb_bands(self, bands, fmax=0.05, climb=True, max_steps=2000, relax_cell=False, cell_factor=None, **kw):
        """
        Nudged elastic bands at once on the device (``neb.NudgedElasticBand``: improved tangents, one FIRE per band).  ``bands``:
        one band (a list of frames, end points included; ``neb.interpolate`` makes one) or a list of bands.  With ``climb`` the
        bands first run to ``fmax`` without a climbing image, then with one; both phases share ``max_steps``.  ``kw``:
        ``spring``, ``fixed``, ``skin``, ``device`` (the object's) and ``dt``, ``dt_max``, ``maxstep``, ``check_every``
        (``run``'s).  Returns (bands, info), info as ``NudgedElasticBand.run`` returns it (``barrier``, ``energies``, ...);
        warns (RuntimeWarning) for every band that did not converge.  ``relax_cell=True``: the images of a band may differ in
        cell and the cells of the interior images move with the atoms (``neb.CellNudgedElasticBand``; ``cell_factor`` is its
        argument, ``fixed`` and ``skin`` are not taken); the returned images carry their cells.
        """
        import warnings
        from .neb import CellNudgedElasticBand, NudgedElasticBand
        if not isinstance(relax_cell, (bool, np.bool_)):
            raise ValueError(f"neb_bands: relax_cell must be True or False, got {relax_cell!r}")
        if relax_cell:
            for k in ("fixed", "skin"):
                if k in kw:
                    raise ValueError(f"neb_bands: {k} is not supported together with relax_cell")
            make = {k: kw.pop(k) for k in ("spring", "device") if k in kw}
            opt = CellNudgedElasticBand(self, bands, cell_factor=cell_factor, **make)
        else:
            if cell_factor is not None:
                raise ValueError("neb_bands: cell_factor needs relax_cell=True")
            make = {k: kw.pop(k) for k in ("spring", "fixed", "skin", "device") if k in kw}
            opt = NudgedElasticBand(self, bands, **make)
        with opt as band:
            info = band.run(max_steps, fmax=fmax, climb=False, **kw)
            if climb:
                left = max_steps - int(info["steps"].max())
                info = band.run(max(left, 0), fmax=fmax, climb=True, **kw)
            out = band.get_images()
        for k, status in enumerate(info["status"]):
            if status != "converged":
                warnings.warn(f"neb_bands: band {k} did not converge ({status} after {info['steps'][k]} steps, criterion "
                              f"{info['criterion'][k]:.3g} eV/A)", RuntimeWarning)
        return out, info

    def monte_carlo(self, atoms_or_list, n_trials, temperature_K, **kw):
        """
        Species-swap Monte Carlo of a batch of frames at once on the device (``mc.MonteCarlo``: fixed positions, every frame
        its own chain and temperature; canonical swaps, or with ``mode="transmute"`` and ``chemical_potentials``
        semi-grand-canonical transmutations).  ``kw``: ``mode``, ``chemical_potentials``, ``swappable``, ``seed``, ``device``
        (the object's) and ``record_every`` (``run``'s).  Returns (frames with their final species, info), info as
        ``MonteCarlo.run`` returns it; warns (RuntimeWarning) for every frame a non-finite energy difference froze.
        """
        import warnings
        from .mc import MonteCarlo
        make = {k: kw.pop(k) for k in ("mode", "chemical_potentials", "swappable", "seed", "device") if k in kw}
        with MonteCarlo(self, atoms_or_list, temperature_K, **make) as mc:
            info = mc.run(n_trials, **kw)
            out = mc.get_atoms()
        for k, status in enumerate(info["status"]):
            if status != "running":
                warnings.warn(f"monte_carlo: frame {k} froze ({status} after {info['trials'][k]} trials)", RuntimeWarning)
        return out, info

    def get_hessian(self, atoms, rows=None, strain=False):
        """Exact second derivatives of the energy on the device (``harmonic.hessian``): H [3N, 3N] (or the rows of ``rows``),
        with ``strain=True`` also the mixed position / strain derivatives, the clamped-ion strain term and the virial."""
        from . import harmonic
        return harmonic.hessian(self, atoms, rows=rows, strain=strain)

    def get_elastic_constants(self, atoms, n=5, d=1.0):
        """
        [C11, C12, C44, B] in GPa (reference: calculator.py:449-467) from the exact second derivatives of the energy, ions
        relaxed (``harmonic.elastic_tensor``).  ``n`` and ``d`` (the reference's number and size of finite distortions) are
        accepted and unused: nothing is sampled.  B = (C11 + 2 C12) / 3 from the same tensor, where the reference fits a
        Birch-Murnaghan equation of state.  A tensor without cubic form in the cell's frame (1e-6 of its largest entry)
        raises ValueError: ``harmonic.elastic_tensor`` gives the full tensor.
        """
        from . import harmonic
        return harmonic.cubic_constants(harmonic.elastic_tensor(self, atoms)["C"])

    def get_phonon_data(self, atoms, n_super=5, disp=0.05, resolution=30, path=None, masses=None):
        """(force_constants, path_data, bands_dict) in the reference's shapes (calculator.py:469-487) from the device Hessian
        of the n_super^3 supercell (``harmonic.band_structure``).  ``disp`` (the reference's finite displacement) is accepted
        and unused.  Masses: ``masses`` ({symbol or Z: amu} or per-atom), else ``atoms.get_masses()`` -- which ASE frames have
        and the package's own ``Atoms`` does not: pass ``masses`` with those (there is no built-in mass table)."""
        from . import harmonic
        return harmonic.band_structure(self, atoms, path=path, n_super=n_super, resolution=resolution, masses=masses)

    def get_phonon_dos(self, atoms, mesh=(20, 20, 20), n_super=5, masses=None, sigma=None, **kwargs):
        """Phonon density of states on a q-mesh (``harmonic.density_of_states``, its dict): ``frequencies`` and ``dos`` (states
        per THz per cell), ``edges`` and ``counts`` (int64 histogram), ``n_imaginary``.  D(q), its eigenvalues and the DOS are
        computed on the device from one Hessian of the n_super^3 supercell.  Where phonopy's ``run_total_dos`` uses the
        tetrahedron method by default, this smears with Gaussians of width ``sigma`` (THz); the mesh is reduced by time
        reversal only.  Masses: as for ``get_phonon_data``."""
        from . import harmonic
        return harmonic.density_of_states(self, atoms, mesh, n_super=n_super, masses=masses, sigma=sigma, **kwargs)

    def get_thermal_properties(self, atoms, temperatures, mesh=(20, 20, 20), n_super=5, masses=None, cutoff_THz=1e-3, **kwargs):
        """Harmonic free energy, internal energy (eV per cell), entropy and heat capacity (eV / K per cell) at ``temperatures``
        (K) from a q-mesh (``harmonic.thermal_properties``, its dict, with ``zero_point_energy`` and ``n_excluded``), on the
        device.  phonopy's ``run_thermal_properties`` reports kJ / mol and J / K / mol; modes at or below ``cutoff_THz`` are
        left out and counted, as phonopy's cutoff_frequency does.  Masses: as for ``get_phonon_data``."""
        from . import harmonic
        return harmonic.thermal_properties(self, atoms, temperatures, mesh, n_super=n_super, masses=masses,
                                           cutoff_THz=cutoff_THz, **kwargs)

    def get_free_energy(self, atoms, temperature_K, masses=None, **kwargs):
        """Anharmonic Helmholtz free energy of ``atoms`` at ``temperature_K`` (K; a list gives one value each) in eV per cell, by
        switching molecular dynamics between the model and an Einstein crystal on the device
        (``free_energy.frenkel_ladd``, whose dict this returns: ``free_energy``, its ``standard_error``, the per-replica
        ``delta_F`` and the ``dissipation``).  Classical nuclei; masses as for ``get_phonon_data``."""
        from . import free_energy
        return free_energy.frenkel_ladd(self, atoms, temperature_K, masses=masses, **kwargs)

    def get_phonon_pdos(self, atoms, mesh=(20, 20, 20), n_super=5, masses=None, sigma=None, by="atom", **kwargs):
        """Projected phonon density of states on a q-mesh (``harmonic.projected_dos``, its dict): ``frequencies``, ``pdos``
        [n_groups, n_samples], ``labels`` and the total ``dos``, grouped ``by`` "atom", "species" or "channel"; eigenvectors,
        smearing and sums on the device (phonopy's ``run_projected_dos``, with Gaussians).  Cells of at most 21 atoms.
        Masses: as for ``get_phonon_data``."""
        from . import harmonic
        return harmonic.projected_dos(self, atoms, mesh, n_super=n_super, masses=masses, sigma=sigma, by=by, **kwargs)

    def get_thermal_displacements(self, atoms, temperatures, mesh=(20, 20, 20), n_super=5, masses=None, cutoff_THz=1e-3, **kwargs):
        """Mean-square thermal displacement tensors at ``temperatures`` (K) from a q-mesh (``harmonic.thermal_displacements``,
        its dict): ``U`` [n_T, N, 3, 3] and ``u_iso`` [n_T, N] in A^2, ``n_excluded`` (phonopy's
        ``run_thermal_displacement_matrices``).  Cells of at most 21 atoms.  Masses: as for ``get_phonon_data``."""
        from . import harmonic
        return harmonic.thermal_displacements(self, atoms, temperatures, mesh, n_super=n_super, masses=masses,
                                              cutoff_THz=cutoff_THz, **kwargs)

    def get_group_velocities(self, atoms, qpoints, n_super=5, masses=None, cutoff_THz=1e-3):
        """Phonon frequencies [nq, 3N] (THz) and group velocities [nq, 3N, 3] (THz A = 100 m / s) at reduced wave vectors
        ``qpoints`` (``harmonic.group_velocities``): Hellmann-Feynman on the device's eigenvectors; inside a degenerate
        cluster of modes only the sum of the velocities is defined.  Masses: as for ``get_phonon_data``."""
        from . import harmonic
        return harmonic.group_velocities(self, atoms, qpoints, n_super=n_super, masses=masses, cutoff_THz=cutoff_THz)
