"""
``MolecularDynamics``: velocity Verlet (NVE) and Langevin (BAOAB, NVT) dynamics of a batch of frames, stepped on the device
(``uf3_md_*`` in ``libuf3hip.so``).  Positions, velocities and forces stay in HBM between steps; the forces are the
evaluator's (``UFCalculator``'s model, its MD route with a neighbour-list skin), the integrator is one fused kernel between
two force calls.  Many small replicas in one batch cost no more machinery than one large frame.

Units: Angstrom, fs, amu, eV, K.  Positions are reported unwrapped (``get_positions(wrap=True)`` wraps a copy); with
``wrap=True`` the object stores them wrapped next to integer image counts (``get_images``) and atoms may cross cell faces:
diffusion, a melt.  ``run(n, msd_every=k)`` samples the mean-squared displacement on the device.  Random numbers
are counter-based (Philox4x32-10 on (atom, absolute step, draw), keyed by the seed), so ``run(60)`` equals
``run(25); run(35)`` and the trajectory does not depend on how the batch is launched.

    md = MolecularDynamics(calc, atoms_list, timestep_fs=1.0, masses={'W': 183.84}, temperature_K=300, friction_per_fs=0.01)
    md.initialize_velocities(300, exact=True)
    rec = md.run(1000, thermo_every=10, stress=True)      # rec['temperature'][k, frame], rec['pressure'], ...

Constant pressure (isotropic Martyna-Tobias-Klein, every frame its own piston): a ``pressure_eV_A3``
makes every ``run`` an NPH run (no friction) or an NPT run (Langevin on the atoms and on the piston); the cells change on
the device and ``dyn.cells`` / ``dyn.volumes`` follow them.

    npt = MolecularDynamics(calc, atoms_list, 1.0, masses=..., temperature_K=300, friction_per_fs=0.01, pressure_eV_A3=0.0,
                            barostat_time_fs=500.0, barostat_friction_per_fs=0.002)

Heat current: ``run(n, flux_every=k)`` samples J = J_conv + J_pot of every frame on the device after
every k-th step; ``heat_flux_autocorrelation`` and ``green_kubo`` turn the series into a thermal conductivity.

    rec = md.run(200000, flux_every=10)
    kappa = green_kubo(rec['heat_flux'][:, 0], 10 * md.timestep_fs, md.volumes[0], 300.0, max_lag=2000)

Diffusion: a wrapping object and the mean-squared displacement of every k-th step, per species and over all atoms.

    dyn = MolecularDynamics(calc, atoms_list, 1.0, masses=..., temperature_K=2500, friction_per_fs=0.01, wrap=True)
    rec = dyn.run(100000, msd_every=10)
    D = diffusion_coefficient(rec['msd_all'][:, 0], 10 * dyn.timestep_fs)             # Angstrom^2 / fs

Each ``run`` starts with one neighbour-list build (it sets the context's skin for its own duration and puts the caller's
back).  A basis without 3-body terms never takes the evaluator's MD route and rebuilds its lists on every step: correct,
only slower.
"""
import ctypes as C
import numbers

import numpy as np

from uf3_amd import _lib
from uf3_amd.forcefield._driver import Driver, check_int, check_real, frames_of
from uf3_amd.data.composition import atomic_numbers, chemical_symbols

ACC = 0.009648533215665327       # eV / (Angstrom amu) -> Angstrom / fs^2
KE_UNIT = 103.64269652680505     # amu Angstrom^2 / fs^2 -> eV
KB = 8.617333262e-5              # eV / K
ASE_TIME_FS = 10.180505          # one ASE time unit in fs (sqrt(KE_UNIT)): ASE velocities / ASE_TIME_FS = Angstrom / fs


EV_PER_A_FS_K_TO_W_PER_M_K = 1.602176634e-19 / (1e-10 * 1e-15)       # eV / (Angstrom fs K) -> W / (m K)


def heat_flux_autocorrelation(J, max_lag):
    """<J(0) . J(t)> of a series J [n, ..., 3] sampled at equal spacing, lags 0 .. ``max_lag``: [max_lag + 1, ...].
    C(k) = 1 / (n - k) sum_t J(t) . J(t + k): the unbiased normalisation, and the mean is NOT subtracted (the heat current
    of an equilibrium run has zero mean; removing a sample mean would bias the Green-Kubo integral).  Computed through a
    zero-padded FFT (NumPy, on the host), which gives the same sums as the direct double loop."""
    J = np.asarray(J, dtype=float)
    if J.ndim < 2 or J.shape[-1] != 3:
        raise ValueError(f"heat_flux_autocorrelation: J must be [n, ..., 3], got {list(J.shape)}")
    n = J.shape[0]
    max_lag = check_int(WHO, "max_lag", max_lag, 0, max(n - 1, 0))
    size = 1
    while size < 2 * n:
        size *= 2
    spec = np.fft.rfft(J, n=size, axis=0)
    corr = np.fft.irfft(spec * np.conj(spec), n=size, axis=0)[:max_lag + 1].sum(axis=-1)
    norm = (n - np.arange(max_lag + 1)).astype(float)
    return corr / norm.reshape((-1,) + (1,) * (corr.ndim - 1))


def green_kubo(J, timestep_fs, volume_A3, temperature_K, max_lag):
    """Running Green-Kubo integral kappa(tau) = 1 / (3 V k_B T^2) int_0^tau <J(0) . J(t)> dt in W / (m K), [max_lag + 1, ...]
    for tau = 0, dt, ..., max_lag dt (trapezoidal rule).  ``J`` [n, ..., 3] in eV A / fs (``run``'s ``heat_flux`` of one
    frame), ``timestep_fs`` the spacing of the SAMPLES (``flux_every`` times the integrator's step), ``volume_A3`` in A^3,
    ``temperature_K`` in K.  Units: (eV A / fs)^2 fs / (A^3 (eV / K) K^2) = eV / (A fs K), times
    1.602176634e-19 J/eV / (1e-10 m/A * 1e-15 s/fs) = 1.602176634e6 gives W / (m K).  The autocorrelation is
    ``heat_flux_autocorrelation``'s (unbiased, mean not subtracted)."""
    dt = check_real(WHO, "timestep_fs", timestep_fs, strict=True)
    vol = check_real(WHO, "volume_A3", volume_A3, strict=True)
    temp = check_real(WHO, "temperature_K", temperature_K, strict=True)
    corr = heat_flux_autocorrelation(J, max_lag)
    integral = np.zeros_like(corr)
    integral[1:] = np.cumsum(0.5 * (corr[1:] + corr[:-1]), axis=0) * dt
    return integral / (3.0 * vol * KB * temp * temp) * EV_PER_A_FS_K_TO_W_PER_M_K


def kinetic_energy(velocities, masses):
    """1/2 sum m v^2 in eV of velocities [N, 3] (Angstrom / fs) and masses [N] (amu)."""
    v = np.asarray(velocities, dtype=float).reshape(-1, 3)
    return 0.5 * float(np.sum(np.asarray(masses, dtype=float) * np.sum(v * v, axis=1))) * KE_UNIT


def temperature(kinetic_energy_eV, n_atoms):
    """2 KE / (3 N k_B), K (3N degrees of freedom, as ASE's ``get_temperature``)."""
    return 2.0 * np.asarray(kinetic_energy_eV, dtype=float) / (3.0 * np.asarray(n_atoms, dtype=float) * KB)


WHO = "MolecularDynamics"


def msd_records(raw, species_counts, first_step, every):
    """The entries ``run(..., msd_every=k)`` adds, from raw records [n, n_frames, 4 S + 4] (``uf3_md_run_msd``: per species
    sum |dr|^2, sum dx, sum dy, sum dz; then sum m dr (3) and sum m) and the atoms of every species in every frame
    ``species_counts`` [n_frames, S]: ``msd`` [n, n_frames, S] the per-species mean (NaN for a species a frame lacks),
    ``msd_all`` [n, n_frames] the mean over all atoms, ``msd_com_removed`` and ``msd_all_com_removed`` of the same two shapes:
    the mean of |dr_i - dr_cm|^2 = (1/N) sum |dr_i|^2 - 2 dr_cm . <dr> + |dr_cm|^2 with the frame's mass-weighted
    dr_cm = sum m dr / sum m, and ``msd_step``."""
    raw = np.asarray(raw, dtype=float)
    cnt = np.asarray(species_counts, dtype=float)
    n_sp = cnt.shape[1]
    if raw.ndim != 3 or raw.shape[1] != cnt.shape[0] or raw.shape[2] != 4 * n_sp + 4:
        raise ValueError(f"msd_records: raw must be [n, {cnt.shape[0]}, {4 * n_sp + 4}], got {list(raw.shape)}")
    per = raw[..., :4 * n_sp].reshape(raw.shape[0], raw.shape[1], n_sp, 4)
    sq, lin = per[..., 0], per[..., 1:]                                      # [n, nf, S], [n, nf, S, 3]
    cm = raw[..., 4 * n_sp:4 * n_sp + 3] / raw[..., 4 * n_sp + 3:]           # [n, nf, 3]
    cm2 = np.sum(cm * cm, axis=-1)
    with np.errstate(invalid="ignore", divide="ignore"):
        n_s = np.where(cnt > 0, cnt, np.nan)[None]                           # [1, nf, S]
        msd = sq / n_s
        com_s = msd - 2.0 * np.einsum("nfd,nfsd->nfs", cm, lin) / n_s + cm2[..., None]
    n_all = cnt.sum(axis=1)[None]
    msd_all = sq.sum(axis=2) / n_all
    com_all = msd_all - 2.0 * np.einsum("nfd,nfd->nf", cm, lin.sum(axis=2)) / n_all + cm2
    return dict(msd=msd, msd_all=msd_all, msd_com_removed=com_s, msd_all_com_removed=com_all,
                msd_step=first_step + every * np.arange(1, raw.shape[0] + 1, dtype=np.int64))


def diffusion_coefficient(msd, sample_time_fs, fit_from=0.5):
    """Einstein's D = slope / 6 in Angstrom^2 / fs of a mean-squared displacement series ``msd`` [n, ...] (Angstrom^2) sampled
    every ``sample_time_fs``: the least-squares slope of a straight line (with intercept) through the samples from fraction
    ``fit_from`` of the record to its end; sample k lies at time (k + 1) ``sample_time_fs``.  Returns an array of the trailing
    shape (a float for a 1-d series)."""
    who = "diffusion_coefficient"
    y = np.asarray(msd, dtype=float)
    dt = check_real(who, "sample_time_fs", sample_time_fs, strict=True)
    frac = check_real(who, "fit_from", fit_from, hi=1.0)
    if y.ndim < 1 or y.shape[0] < 2:
        raise ValueError(f"{who}: msd must hold at least two samples along its first axis, got {list(y.shape)}")
    lo = min(int(np.floor(frac * y.shape[0])), y.shape[0] - 2)
    t = dt * np.arange(lo + 1, y.shape[0] + 1, dtype=float)
    tc = t - t.mean()
    yy = y[lo:]
    slope = np.tensordot(tc, yy - yy.mean(axis=0), axes=(0, 0)) / np.dot(tc, tc)
    return slope / 6.0 if np.ndim(slope) else float(slope) / 6.0


def resolve_masses(frames, masses=None):
    """Masses [N] (amu) of the concatenated frames from ``{symbol or Z: amu}``, a per-atom array, or ``get_masses()`` of the
    frames (real ASE objects).  There is no built-in mass table: anything else raises ``ValueError`` naming the species that
    lack a mass."""
    frames = frames_of(WHO, frames)
    z = np.concatenate([np.asarray(a.get_atomic_numbers(), dtype=np.int64).reshape(-1) for a in frames])
    if masses is None:
        if all(hasattr(a, "get_masses") for a in frames):
            m = np.concatenate([np.asarray(a.get_masses(), dtype=float).reshape(-1) for a in frames])
        else:
            missing = sorted({chemical_symbols[int(q)] for q in z})
            raise ValueError(f"MolecularDynamics: no masses for {', '.join(missing)}: pass masses={{symbol: amu}} or a "
                             "per-atom array (there is no built-in mass table)")
    elif isinstance(masses, dict):
        table = {}
        for key, value in masses.items():
            zk = int(key) if isinstance(key, numbers.Integral) else atomic_numbers.get(str(key))
            if zk is None:
                raise ValueError(f"MolecularDynamics: unknown element {key!r} in masses")
            table[zk] = float(value)
        missing = sorted({int(q) for q in z} - set(table))
        if missing:
            raise ValueError(f"MolecularDynamics: no mass for {', '.join(chemical_symbols[q] for q in missing)}")
        m = np.array([table[int(q)] for q in z], dtype=float)
    else:
        m = np.asarray(masses, dtype=float).reshape(-1)
        if m.shape != z.shape:
            raise ValueError(f"MolecularDynamics: {m.size} masses for {z.size} atoms")
    if m.shape != z.shape:
        raise ValueError(f"MolecularDynamics: {m.size} masses for {z.size} atoms")
    if not np.all(np.isfinite(m)) or np.any(m <= 0):
        raise ValueError("MolecularDynamics: masses must be positive and finite")
    return np.ascontiguousarray(m)


def thermo_records(raw, n_atoms, volumes, first_step, every, stress=False):
    """The dict ``run`` returns from raw records [n_rec, n_frames, 2 or 14] ([PE, KE] or [PE, KE, W (6), K (6)], eV): step,
    potential_energy, kinetic_energy, temperature [n_rec, n_frames]; with stress also stress [n_rec, n_frames, 6] =
    (W - K) / V (ASE's include_ideal_gas convention, the sign of ``UFCalculator.get_stress``; NaN for frames without a volume)
    and pressure = -trace / 3."""
    raw = np.asarray(raw, dtype=float)
    n_rec = raw.shape[0]
    out = dict(step=first_step + every * np.arange(1, n_rec + 1, dtype=np.int64),
               potential_energy=raw[..., 0].copy(), kinetic_energy=raw[..., 1].copy(),
               temperature=temperature(raw[..., 1], np.asarray(n_atoms, dtype=float)[None, :]))
    if stress:
        vol = np.asarray(volumes, dtype=float)
        inv = np.where(vol > 0, 1.0 / np.where(vol > 0, vol, 1.0), np.nan)
        s = (raw[..., 2:8] - raw[..., 8:14]) * inv[None, :, None]
        out["stress"] = s
        out["pressure"] = -(s[..., 0] + s[..., 1] + s[..., 2]) / 3.0
    return out


def npt_records(raw, n_atoms, first_step, every):
    """The dict a constant-pressure ``run`` returns from raw records [n_rec, n_frames, 17] ([PE, KE, W (6), K (6), V, s, H]):
    ``thermo_records``' entries with the stress and pressure of each step's own volume, and volume, cell_scale, conserved."""
    raw = np.asarray(raw, dtype=float)
    out = thermo_records(raw[..., :14], n_atoms, np.ones(raw.shape[1]), first_step, every, stress=True)
    vol = raw[..., 14]
    out["stress"] = out["stress"] / vol[..., None]
    out["pressure"] = out["pressure"] / vol
    out["volume"] = vol.copy()
    out["cell_scale"] = raw[..., 15].copy()
    out["conserved"] = raw[..., 16].copy()
    return out


class MolecularDynamics(Driver):
    """Velocity Verlet / Langevin / constant-pressure dynamics of a batch of frames on the device (module text above).

    Atoms outside the cell.  ``wrap=True`` (or ``dyn.wrap = True``): the object stores wrapped positions and int32 image counts;
    its position is ``pos + images @ cell`` with the current cell, which is what ``get_positions()`` and ``get_atoms()`` return.
    Positions are folded into the cell on the device in front of every neighbour-list build made for the object (and in front
    of every evaluation when the lists are rebuilt every time: ``skin=0``, 2-body bases), never between a build and the steps on
    its lists, so no evaluation sees an atom farther outside its cell than it has moved since the last wrap (at most skin / 2)
    and atoms may cross cell faces freely.  A wrap rounds: the last bits of a wrapping trajectory depend on where the lists
    were built (the skin, the run boundaries); it is deterministic for a given sequence of calls, and ``run(60)`` agrees with
    ``run(25); run(35)`` to 1e-10, not bit for bit.  ``set_positions`` takes positions as given and zeroes the image counts;
    turning ``wrap`` off folds the image counts back into the positions.

    ``wrap=False``, the default, for which the hazard remains: positions are kept unwrapped and go to the evaluator as they
    are, and the evaluator takes the reference's finite image range around the positions as given (``include/uf3_hip.h``, above
    ``uf3_md_create``).  An atom that leaves its cell during such a run loses the interactions that range no
    longer reaches from where it is: energies and forces are then ``evaluate_frames``' of the unwrapped positions, not the
    wrapped crystal's.  Use ``wrap=True`` for anything that diffuses."""
    KIND, WHO = "md", WHO

    def __init__(self, calculator, atoms_or_list, timestep_fs, masses=None, temperature_K=0.0, friction_per_fs=0.0, seed=0,
                 skin=0.5, device=None, pressure_eV_A3=None, barostat_time_fs=None, barostat_friction_per_fs=0.0,
                 piston_temperature_K=None, wrap=False):
        # every argument is checked before the device is touched
        wrap = self._check_wrap(wrap)
        self.timestep_fs = check_real(WHO, "timestep_fs", timestep_fs, strict=True)
        self.temperature_K = check_real(WHO, "temperature_K", temperature_K)
        self.friction_per_fs = check_real(WHO, "friction_per_fs", friction_per_fs)
        self.seed = check_int(WHO, "seed", seed, 0, (1 << 64) - 1)
        self.skin = check_real(WHO, "skin", skin, hi=4.0)
        self.pressure_eV_A3 = self.barostat_time_fs = self.piston_temperature_K = None
        self.barostat_friction_per_fs = 0.0
        self._check_barostat(pressure_eV_A3, barostat_time_fs, barostat_friction_per_fs, piston_temperature_K)
        self._list = isinstance(atoms_or_list, (list, tuple))
        self.frames = frames_of(WHO, atoms_or_list)
        self.masses = resolve_masses(self.frames, masses)
        if self.pressure_eV_A3 is not None:
            for k, a in enumerate(self.frames):
                if not np.all(np.asarray(a.get_pbc() if hasattr(a, "get_pbc") else a.pbc, dtype=bool)):
                    raise ValueError(f"MolecularDynamics: frame {k} is not periodic along all three axes: it cannot be run at "
                                     "a pressure (and barostatted and positions-only frames do not mix in one object)")
                if not abs(np.linalg.det(np.asarray(a.get_cell(), dtype=float).reshape(3, 3))) > 0:
                    raise ValueError(f"MolecularDynamics: frame {k} has a singular cell")
        vel = None
        if all(hasattr(a, "get_velocities") for a in self.frames):
            vel = np.concatenate([np.asarray(a.get_velocities(), dtype=float).reshape(-1, 3) for a in self.frames]) / ASE_TIME_FS
            if not np.all(np.isfinite(vel)):
                raise ValueError("MolecularDynamics: velocities must be finite")
        self.calculator = calculator
        self._batch = _lib.FrameBatch(self.frames)
        if not np.all(np.isfinite(self._batch.pos)):
            raise ValueError("MolecularDynamics: positions must be finite")
        self.n_atoms = np.diff(self._batch.offsets).astype(np.int64)
        self._cell_scale = np.ones(self._batch.n_frames)
        self._grade_w_host = self._grade_w_dev = None
        vel = None if vel is None else np.ascontiguousarray(vel)
        self._create(calculator, device, [_lib._p(self._batch.pos), _lib._p(vel), _lib._p(self._batch.z), _lib._p(self.masses)])
        if wrap:
            self.wrap = True

    @staticmethod
    def _check_wrap(value):
        if not isinstance(value, (bool, np.bool_)):
            raise ValueError(f"MolecularDynamics: wrap must be True or False, got {value!r}")
        return bool(value)

    @property
    def wrap(self):
        """Whether the object wraps (class text).  Setting it True wraps now and in front of every list build from then on;
        setting it False folds the image counts into the positions."""
        return getattr(self, "_wrap", False)

    @wrap.setter
    def wrap(self, value):
        value = self._check_wrap(value)
        self.ctx.check(self.ctx.lib.uf3_md_set_wrap(self._live(), int(value)))
        self._wrap = value

    def _check_barostat(self, pressure, tau, gamma_p, t_piston):
        """The constant-pressure arguments, checked as a set (nothing touches the device); returns what a run passes on."""
        if pressure is None:
            if tau is not None or t_piston is not None or check_real(WHO, "barostat_friction_per_fs", gamma_p) != 0.0:
                raise ValueError("MolecularDynamics: barostat_time_fs, barostat_friction_per_fs and piston_temperature_K need a "
                                 "pressure_eV_A3")
            return None
        p = check_real(WHO, "pressure_eV_A3", pressure, lo=None)
        if tau is None:
            raise ValueError("MolecularDynamics: pressure_eV_A3 needs a barostat_time_fs")
        tau = check_real(WHO, "barostat_time_fs", tau, strict=True)
        gamma_p = check_real(WHO, "barostat_friction_per_fs", gamma_p)
        t_bath = check_real(WHO, "temperature_K", self.temperature_K)
        if t_piston is None:
            if not t_bath > 0:
                raise ValueError("MolecularDynamics: with temperature_K = 0 the piston mass needs a piston_temperature_K > 0")
            t_p = t_bath
        else:
            t_p = check_real(WHO, "piston_temperature_K", t_piston, strict=True)
        self.pressure_eV_A3, self.barostat_time_fs, self.barostat_friction_per_fs, self.piston_temperature_K = p, tau, gamma_p, t_piston
        return p, tau, gamma_p, t_p

    # ---- state ------------------------------------------------------------------------------------------------------------
    @property
    def step(self):
        s = C.c_int64()
        self.ctx.check(self.ctx.lib.uf3_md_info(self._live(), C.byref(s), None, None))
        return s.value

    @property
    def cells(self):
        """[n_frames, 3, 3] the current cells (those of the frames given, unless the object runs at a pressure)."""
        return self._batch.cells.copy()

    @property
    def volumes(self):
        """[n_frames] the current volumes."""
        return np.abs(np.linalg.det(self._batch.cells))

    @property
    def cell_scales(self):
        """[n_frames] the current cells' scale s relative to the frames given."""
        return self._cell_scale.copy()

    @property
    def strain_rates(self):
        """[n_frames] the pistons' v_eps = d ln s / dt, 1/fs (0 without a pressure)."""
        out = np.zeros(self._batch.n_frames)
        self.ctx.check(self.ctx.lib.uf3_md_get_cells(self._live(), None, None, _lib._p(out)))
        return out

    def _fetch_cells(self):
        # (in place: the C struct of the batch points at this array)
        self.ctx.lib.uf3_md_get_cells(self._live(), _lib._p(self._batch.cells), _lib._p(self._cell_scale), None)

    def _get(self, which):
        atoms = ((self._batch.n_atoms, 3), float)
        return self._fetch(dict(pos=atoms, vel=atoms, forces=atoms, energies=((self._batch.n_frames,), float)), (which,))[which]

    def get_positions(self, wrap=False):
        """[N, 3] Angstrom, frames concatenated; unwrapped unless ``wrap`` (into the cell along periodic directions)."""
        pos = self._get("pos")
        if wrap:
            off = self._batch.offsets
            for k in range(self._batch.n_frames):
                per = self._batch.pbc[k].astype(bool)
                if not per.any():
                    continue
                cell = self._batch.cells[k]
                frac = pos[off[k]:off[k + 1]] @ np.linalg.inv(cell)
                frac[:, per] -= np.floor(frac[:, per])
                pos[off[k]:off[k + 1]] = frac @ cell
        return pos

    def get_images(self):
        """[N, 3] int: the image counts of a wrapping object, position = stored position + images @ cell (zeros with
        ``wrap=False``)."""
        img = np.zeros((self._batch.n_atoms, 3), dtype=np.int32)
        self.ctx.check(self.ctx.lib.uf3_md_get_wrapped(self._live(), None, _lib._p(img)))
        return img.astype(np.int64)

    def set_msd_origin(self, positions=None):
        """The origin of ``run(..., msd_every=k)``'s displacements: [N, 3] Angstrom, default the current (unwrapped) positions.
        A sampling run of an object that never got one starts from where that run starts."""
        p = None if positions is None else self._state_array("positions", positions)
        self.ctx.check(self.ctx.lib.uf3_md_msd_origin(self._live(), _lib._p(p)))

    def get_velocities(self):
        """[N, 3] Angstrom / fs."""
        return self._get("vel")

    def get_forces(self):
        """[N, 3] eV / Angstrom at the current positions."""
        return self._get("forces")

    def get_potential_energies(self):
        """[n_frames] eV at the current positions."""
        return self._get("energies")

    def get_atoms(self):
        """The frames at the current (unwrapped) positions: a list when a list was given, else one object."""
        from uf3_amd.data.atoms import Atoms
        pos, off = self.get_positions(), self._batch.offsets
        out = [Atoms(numbers=a.get_atomic_numbers(), positions=pos[off[k]:off[k + 1]], cell=self._batch.cells[k].copy(), pbc=a.get_pbc())
               for k, a in enumerate(self.frames)]
        return out if self._list else out[0]

    def _state_array(self, name, x):
        a = np.ascontiguousarray(np.asarray(x, dtype=float))
        if a.shape != (self._batch.n_atoms, 3):
            raise ValueError(f"MolecularDynamics: {name} must be [{self._batch.n_atoms}, 3], got {np.shape(x)}")
        if not np.all(np.isfinite(a)):
            raise ValueError(f"MolecularDynamics: {name} must be finite")
        return a

    def set_positions(self, positions):
        """[N, 3] Angstrom (frames concatenated); the forces are evaluated again before the next step."""
        p = self._state_array("positions", positions)
        self.ctx.check(self.ctx.lib.uf3_md_set_state(self._live(), _lib._p(p), None))

    def set_velocities(self, velocities):
        """[N, 3] Angstrom / fs (frames concatenated)."""
        v = self._state_array("velocities", velocities)
        self.ctx.check(self.ctx.lib.uf3_md_set_state(self._live(), None, _lib._p(v)))

    # ---- dynamics ---------------------------------------------------------------------------------------------------------
    def initialize_velocities(self, temperature_K, seed=None, exact=False):
        """Maxwell-Boltzmann velocities at ``temperature_K`` (Philox stream of ``seed``, default the object's, at the current
        step), each frame's centre-of-mass velocity removed; ``exact``: each frame rescaled to exactly ``temperature_K``."""
        t = check_real(WHO, "temperature_K", temperature_K)
        s = self.seed if seed is None else check_int(WHO, "seed", seed, 0, (1 << 64) - 1)
        self.ctx.check(self.ctx.lib.uf3_md_init_velocities(self._live(), t, s, int(bool(exact))))

    def run(self, n_steps, thermo_every=0, stress=False, flux_every=0, grade_every=0, grade_stop=None, msd_every=0):
        """``n_steps`` steps (Langevin when ``friction_per_fs`` > 0, else NVE; at a pressure NPT / NPH).  Returns the thermo
        records of every ``thermo_every``-th step (see ``thermo_records``; empty arrays when ``thermo_every`` is 0).  At a
        pressure the records always carry stress and pressure (of that step's volume), volume, cell_scale and conserved.
        ``flux_every`` > 0: the heat current of every frame after every ``flux_every``-th step, sampled on the device from the
        closed state (``uf3_md_run_flux``): ``heat_flux_convective``, ``heat_flux_potential`` and their sum ``heat_flux``
        [n_records, n_frames, 3] in eV A / fs, and ``flux_step``.  The trajectory and the thermo records do not depend on it.
        Not at a pressure: that raises ``UF3Error`` (UF3_EINVAL).
        ``grade_every`` > 0: after every ``grade_every``-th step the extrapolation grades of the closed state
        (``uf3_md_run_grade``; ``UFCalculator.get_site_grades`` for what they are, of the WRAPPED frame): ``grade``
        [n_samples, n_frames] the largest site grade of each frame, ``grade_atom`` the frame-local index of its atom,
        ``grade_step``, and ``steps_done``.  ``grade_stop`` > 0: the run ends after the first sample in which any frame's
        ``grade`` exceeds it -- the whole batch stops; ``steps_done`` steps were made, every record is cut to them, the state is
        that of ``run(steps_done)`` and a later ``run`` goes on from it.  The trajectory and the thermo records do not depend on
        the sampling.  W is the calculator's ``model.whitening()`` (``ValueError`` without a posterior), uploaded once per
        object.  Not at a pressure and not together with ``flux_every``: ``UF3Error`` (UF3_EINVAL).
        ``msd_every`` > 0: after every ``msd_every``-th step the mean-squared displacement of the closed state from the origin
        (``set_msd_origin``; ``uf3_md_run_msd``), summed on the device without atomics: ``msd`` [n_samples, n_frames, S] per
        species of the basis (ascending atomic number; NaN for a species a frame lacks), ``msd_all`` [n_samples, n_frames],
        ``msd_com_removed`` and ``msd_all_com_removed`` (the frame's mass-weighted centre-of-mass displacement taken out),
        ``msd_step`` and the raw sums ``msd_sums`` (``msd_records``).  Needs ``wrap=True`` as soon as atoms may leave their cell.
        The trajectory and the thermo records do not depend on it.  Not at a pressure and not together with ``flux_every`` or
        ``grade_every``: ``UF3Error`` (UF3_EINVAL)."""
        n_steps = check_int(WHO, "n_steps", n_steps)
        every = check_int(WHO, "thermo_every", thermo_every)
        flux_every = check_int(WHO, "flux_every", flux_every)
        grade_every = check_int(WHO, "grade_every", grade_every)
        grade_stop = 0.0 if grade_stop is None else check_real(WHO, "grade_stop", grade_stop, lo=None)
        msd_every = check_int(WHO, "msd_every", msd_every)
        pressure = getattr(self, "pressure_eV_A3", None)        # (a bare object, as tests/test_md_host.py makes, has no barostat)
        if flux_every and pressure is not None:
            raise _lib.UF3Error(1, "uf3_md_run_flux: the heat current is sampled at constant volume only (flux_every with "
                                   "pressure_eV_A3)")
        if grade_every and pressure is not None:
            raise _lib.UF3Error(1, "uf3_md_run_grade: grades are sampled at constant volume only (grade_every with "
                                   "pressure_eV_A3)")
        if grade_every and flux_every:
            raise _lib.UF3Error(1, "uf3_md_run_grade: grade_every and flux_every do not go into one run")
        if msd_every and pressure is not None:
            raise _lib.UF3Error(1, "uf3_md_run_msd: the mean-squared displacement is sampled at constant volume only (msd_every "
                                   "with pressure_eV_A3)")
        if msd_every and (flux_every or grade_every):
            raise _lib.UF3Error(1, "uf3_md_run_msd: msd_every does not go into one run with flux_every or grade_every")
        w_host = self.calculator.model.whitening() if grade_every else None    # (the ValueError, before anything touches the device)
        dt = check_real(WHO, "timestep_fs", self.timestep_fs, strict=True)
        temp = check_real(WHO, "temperature_K", self.temperature_K)
        gamma = check_real(WHO, "friction_per_fs", self.friction_per_fs)
        skin = check_real(WHO, "skin", self.skin, hi=4.0)
        seed = check_int(WHO, "seed", self.seed, 0, (1 << 64) - 1)
        baro = self._check_barostat(pressure, getattr(self, "barostat_time_fs", None), getattr(self, "barostat_friction_per_fs", 0.0),
                                    getattr(self, "piston_temperature_K", None))
        handle, lib, first = self._live(), self.ctx.lib, self.step
        n_frames, n_rec = self._batch.n_frames, n_steps // every if every else 0
        ring = lambda a: _lib._p(a) if len(a) else None                             # noqa: E731 (no record due: no buffer)
        if baro is not None:
            raw = np.zeros((n_rec, n_frames, 17))
            try:
                self.ctx.check(lib.uf3_md_run_npt(handle, n_steps, dt, temp, gamma, *baro, seed, skin, every, ring(raw)))
            finally:
                self._fetch_cells()
            return npt_records(raw, self.n_atoms, first, max(every, 1))
        raw = np.zeros((n_rec, n_frames, 14 if stress else 2))
        args = (handle, n_steps, dt, temp, gamma, seed, skin, every, int(bool(stress)), ring(raw))
        done = C.c_int64(n_steps)
        if flux_every:
            fl = np.zeros((n_steps // flux_every, n_frames, 2, 3))
            self.ctx.check(lib.uf3_md_run_flux(*args, flux_every, ring(fl)))
        elif grade_every:
            gr = np.zeros((n_steps // grade_every, n_frames, 2))
            self.ctx.check(lib.uf3_md_run_grade(*args, self._grade_w(w_host), grade_every, grade_stop, ring(gr), C.byref(done)))
        elif msd_every:
            ms = np.zeros((n_steps // msd_every, n_frames, 4 * self._dbasis.n_species + 4))
            self.ctx.check(lib.uf3_md_run_msd(*args, msd_every, ring(ms)))
        else:
            self.ctx.check(lib.uf3_md_run(*args))
        done = done.value                   # (fewer than asked only when a grade sample stopped the run: every record is cut to them)
        out = thermo_records(raw[:done // every if every else 0], self.n_atoms, self.volumes, first, max(every, 1), stress)
        if flux_every:
            out["heat_flux_convective"] = fl[:, :, 0].copy()
            out["heat_flux_potential"] = fl[:, :, 1].copy()
            out["heat_flux"] = fl[:, :, 0] + fl[:, :, 1]
            out["flux_step"] = first + flux_every * np.arange(1, len(fl) + 1, dtype=np.int64)
        elif grade_every:
            gr = gr[:done // grade_every]
            out["grade"] = gr[:, :, 0].copy()
            out["grade_atom"] = gr[:, :, 1].astype(np.int64)
            out["grade_step"] = first + grade_every * np.arange(1, len(gr) + 1, dtype=np.int64)
            out["steps_done"] = done
        elif msd_every:
            out.update(msd_records(ms, self._species_counts(), first, msd_every))
            out["msd_sums"] = ms
        return out

    # ---- switching (free energies: uf3_amd.forcefield.free_energy) ----------------------------------------------------------
    def _per_atom_spring(self, spring):
        """``spring`` (None, a scalar, ``{symbol or Z: k}`` or [N]) as the library takes it: None or float64 [N], eV / A^2."""
        if spring is None:
            return None
        if isinstance(spring, dict):
            table = {}
            for key, value in spring.items():
                zk = int(key) if isinstance(key, numbers.Integral) else atomic_numbers.get(str(key))
                if zk is None:
                    raise ValueError(f"MolecularDynamics: unknown element {key!r} in spring")
                table[zk] = check_real(WHO, f"spring[{key!r}]", value)
            missing = sorted({int(q) for q in self._batch.z} - set(table))
            if missing:
                raise ValueError(f"MolecularDynamics: no spring for {', '.join(chemical_symbols[q] for q in missing)}")
            return np.array([table[int(q)] for q in self._batch.z], dtype=float)
        if np.ndim(spring) == 0:
            k = check_real(WHO, "spring", spring)               # (refused before the batch is looked at)
            return np.full(self._batch.n_atoms, k)
        k = np.ascontiguousarray(np.asarray(spring, dtype=float).reshape(-1))
        if k.size != self._batch.n_atoms:
            raise ValueError(f"MolecularDynamics: {k.size} springs for {self._batch.n_atoms} atoms")
        if not np.all(np.isfinite(k)) or np.any(k < 0):
            raise ValueError("MolecularDynamics: spring must be finite and >= 0")
        return k

    def set_reference(self, positions=None, spring=None):
        """The Einstein crystal ``switch`` couples the model to: reference sites ``positions`` [N, 3] Angstrom (default the
        current positions) and spring constants ``spring`` in eV / A^2: a scalar, ``{symbol: k}`` or a per-atom array; None is
        no spring at all, which leaves the scaled model alone (reversible scaling).  Not for a wrapping object and not at a
        pressure (``UF3Error``, UF3_EINVAL)."""
        k = self._per_atom_spring(spring)
        p = None if positions is None else self._state_array("positions", positions)
        self._refuse_switch("uf3_md_set_reference")
        self.ctx.check(self.ctx.lib.uf3_md_set_reference(self._live(), _lib._p(p), _lib._p(k)))
        self.spring = k

    def _refuse_switch(self, who):
        # (the library knows a wrapping object and one that has run at a pressure; one that only will is known here)
        if getattr(self, "pressure_eV_A3", None) is not None:
            raise _lib.UF3Error(1, f"{who}: the object runs at a pressure: a switch is made at constant volume")

    def switch(self, n_steps, lambda_start, lambda_end, schedule="smooth", temperatures_K=None, fix_com=True, every=0):
        """``n_steps`` steps on H(lambda) = K + lambda U_uf3 + (1 - lambda) U_E, U_E the Einstein crystal of ``set_reference``,
        with lambda moving from ``lambda_start`` to ``lambda_end`` (scalars or one value per frame, in [0, 1]) along
        ``schedule``: ``"linear"``, ``"smooth"`` (``free_energy.switching_schedule``) or ``n_steps + 1`` values in [0, 1], the
        fraction of the way at every state of the run.  ``temperatures_K``: one value per frame (default the object's for all);
        the integrator, friction, seed and step counter are ``run``'s.  ``fix_com`` keeps every frame's momentum where
        ``initialize_velocities`` put it (force and noise are projected).  Returns ``work`` [n_frames], the switching work
        sum (lambda(j + 1) - lambda(j)) (D(j) + D(j + 1)) / 2 with D = U_uf3 - U_E, accumulated on the device, and the records
        of every ``every``-th step, each [n_records, n_frames]: ``lambda``, ``potential_energy`` (U_uf3), ``einstein_energy``,
        ``kinetic_energy``, ``work_so_far``; and ``step``.  eV throughout."""
        from uf3_amd.forcefield.free_energy import switching_schedule
        n_steps = check_int(WHO, "n_steps", n_steps)
        every = check_int(WHO, "every", every)
        if not isinstance(fix_com, (bool, np.bool_)):
            raise ValueError(f"MolecularDynamics: fix_com must be True or False, got {fix_com!r}")
        lam = []
        for name, value in (("lambda_start", lambda_start), ("lambda_end", lambda_end)):
            a = np.asarray(value, dtype=float)
            if a.ndim > 1 or not np.all(np.isfinite(a)) or np.any(a < 0) or np.any(a > 1):
                raise ValueError(f"MolecularDynamics: {name} must be a number or one per frame, finite and in [0, 1], got {value!r}")
            lam.append(a)
        if isinstance(schedule, str):
            sched = switching_schedule(n_steps, schedule)
        else:
            sched = np.ascontiguousarray(np.asarray(schedule, dtype=float))
            if sched.shape != (n_steps + 1,):
                raise ValueError(f"MolecularDynamics: schedule must hold n_steps + 1 = {n_steps + 1} values, got {list(sched.shape)}")
            if not np.all(np.isfinite(sched)) or np.any(sched < 0) or np.any(sched > 1):
                raise ValueError("MolecularDynamics: schedule entries must be finite and in [0, 1]")
        dt = check_real(WHO, "timestep_fs", self.timestep_fs, strict=True)
        gamma = check_real(WHO, "friction_per_fs", self.friction_per_fs)
        skin = check_real(WHO, "skin", self.skin, hi=4.0)
        seed = check_int(WHO, "seed", self.seed, 0, (1 << 64) - 1)
        temps = np.asarray(self.temperature_K if temperatures_K is None else temperatures_K, dtype=float)
        if temps.ndim > 1 or not np.all(np.isfinite(temps)) or np.any(temps < 0):
            raise ValueError(f"MolecularDynamics: temperatures_K must be a number or one per frame, finite and >= 0, got {temperatures_K!r}")
        n_frames = self._batch.n_frames
        per_frame = []
        for name, a in (("lambda_start", lam[0]), ("lambda_end", lam[1]), ("temperatures_K", temps)):
            if a.ndim == 1 and a.size != n_frames:
                raise ValueError(f"MolecularDynamics: {name} holds {a.size} values for {n_frames} frames")
            per_frame.append(np.ascontiguousarray(np.broadcast_to(a, (n_frames,)), dtype=float))
        lam_a, lam_b, temps = per_frame
        self._refuse_switch("uf3_md_run_switch")
        handle, lib, first = self._live(), self.ctx.lib, self.step
        raw = np.zeros((n_steps // every if every else 0, n_frames, 5))
        work = np.zeros(n_frames)
        self.ctx.check(lib.uf3_md_run_switch(handle, n_steps, dt, _lib._p(temps), gamma, seed, skin, _lib._p(lam_a), _lib._p(lam_b),
                                             _lib._p(sched), int(bool(fix_com)), every, _lib._p(raw) if len(raw) else None,
                                             _lib._p(work)))
        out = {"work": work, "step": first + max(every, 1) * np.arange(1, len(raw) + 1, dtype=np.int64)}
        for k, name in enumerate(("lambda", "potential_energy", "einstein_energy", "kinetic_energy", "work_so_far")):
            out[name] = raw[..., k].copy()
        return out

    def _species_counts(self):
        """[n_frames, S] the atoms of every species of the basis (ascending atomic number) in every frame."""
        zs = [atomic_numbers[e] for e in self.calculator.bspline_config.chemical_system.element_list]
        off = self._batch.offsets
        return np.array([[int(np.sum(self._batch.z[off[k]:off[k + 1]] == q)) for q in zs] for k in range(self._batch.n_frames)])

    def _grade_w(self, w_host):
        """Device address of the whitening matrix: uploaded once per object (again after a refit made a new one)."""
        if self._grade_w_host is not w_host:
            import torch
            n_feat = _lib.device_basis(self.calculator.bspline_config, self.ctx).n_feat
            if w_host.shape != (n_feat, n_feat):
                raise ValueError("MolecularDynamics: the model's whitening matrix is not of the calculator's basis")
            self._grade_w_dev = torch.from_numpy(np.ascontiguousarray(w_host, dtype=np.float64)).to(torch.device("cuda", self.ctx.device))
            torch.cuda.synchronize(self._grade_w_dev.device)
            self._grade_w_host = w_host
        return C.c_void_p(self._grade_w_dev.data_ptr())
