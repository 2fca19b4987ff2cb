"""
``MonteCarlo``: species-swap Monte Carlo of a batch of frames on the device (``uf3_mc_*`` in ``libuf3hip.so``).  The positions
are fixed (lattice Monte Carlo on relaxed or MD-sampled positions); what changes is which species sits on which site.  Every
frame is its own Markov chain with its own temperature, so one batch can be a temperature ladder; a trial costs the energy
terms that contain the one or two atoms it touches, not an evaluation of the frame.

``mode="swap"`` (canonical): two atoms of the frame exchange their species; the composition is conserved.
``mode="transmute"`` (semi-grand canonical): one atom takes another of the species that have a finite chemical potential in
``chemical_potentials`` ({symbol: eV}; ``-inf`` or a missing symbol excludes a species), accepted on
``dE - (mu_new - mu_old)``.

    with MonteCarlo(calc, frames, temperature_K=[300, 600, 900], seed=7) as mc:
        rec = mc.run(200_000, record_every=1000)       # rec["energy"][k, frame], rec["composition"][k, frame, species]
        ordered = mc.get_atoms()
    alpha = short_range_order(ordered[0], r_shell=2.9)  # Warren-Cowley parameters of the first shell

Random numbers are counter-based (Philox4x32-10 on (frame, absolute trial), keyed by the seed): ``run(a); run(b)`` equals
``run(a + b)`` bit for bit, and a frame's chain does not depend on the batch around it.  Hybrid MC / MD: alternate with
``md.MolecularDynamics`` through ``set_positions`` (which rebuilds the neighbour table).
"""
import numbers

import numpy as np

from uf3_amd import _lib
from uf3_amd.forcefield._driver import Driver, check_int, check_mask, frames_of
from uf3_amd.data.composition import atomic_numbers, chemical_symbols

KB = 8.617333262e-5              # eV / K
MODES = {"swap": 0, "transmute": 1}
STATUS = {0: "running", 2: "nonfinite"}
WHO = "MonteCarlo"


def _temperatures(temperature_K, n_frames):
    try:
        t = np.asarray(temperature_K, dtype=float)
    except (TypeError, ValueError):
        raise ValueError("MonteCarlo: temperature_K must be a number or one number per frame") from None
    if t.ndim == 0:
        t = np.full(n_frames, float(t))
    t = t.reshape(-1)
    if t.size != n_frames:
        raise ValueError(f"MonteCarlo: {t.size} temperatures for {n_frames} frames")
    if not np.all(np.isfinite(t)) or np.any(t < 0):
        raise ValueError(f"MonteCarlo: temperature_K must be finite and >= 0, got {temperature_K!r}")
    return np.ascontiguousarray(t)


def _species_index(element_list, key, what):
    """Index into the basis' element list of a symbol or an atomic number."""
    symbol = chemical_symbols[int(key)] if isinstance(key, numbers.Integral) and 0 < int(key) < len(chemical_symbols) else str(key)
    if symbol not in atomic_numbers:
        raise ValueError(f"MonteCarlo: unknown element {key!r} in {what}")
    if symbol not in element_list:
        raise ValueError(f"MonteCarlo: {symbol} in {what} is not a species of the model ({', '.join(element_list)})")
    return list(element_list).index(symbol)


def _chemical_potentials(mode, chemical_potentials, element_list):
    """[S] in the order of the element list (-inf: species not allowed), or None in swap mode."""
    if mode == "swap":
        if chemical_potentials is not None:
            raise ValueError("MonteCarlo: chemical_potentials belong to mode='transmute' (swaps conserve the composition)")
        return None
    if not isinstance(chemical_potentials, dict) or not chemical_potentials:
        raise ValueError("MonteCarlo: mode='transmute' needs chemical_potentials={symbol: eV}")
    mu = np.full(len(element_list), -np.inf)
    for key, value in chemical_potentials.items():
        k = _species_index(element_list, key, "chemical_potentials")
        try:
            x = float(value)
        except (TypeError, ValueError):
            raise ValueError(f"MonteCarlo: chemical potential of {key!r} must be a number") from None
        if np.isnan(x) or x == np.inf:
            raise ValueError(f"MonteCarlo: chemical potential of {key!r} must be finite or -inf, got {value!r}")
        mu[k] = x
    if np.sum(np.isfinite(mu)) < 2:
        raise ValueError("MonteCarlo: mode='transmute' needs at least two species with a finite chemical potential")
    return np.ascontiguousarray(mu)


def run_records(raw, first_trial, every):
    """The dict ``run`` returns from raw records [n_rec, n_frames, 3 + S] ([E, accepted, trials, atoms of each species]):
    ``trial`` [n_rec] (absolute index of the object's trial counter after the record's trial), ``energy`` [n_rec, n_frames]
    (eV), ``accepted`` and ``trials`` [n_rec, n_frames] (int64, totals of the object so far), ``composition``
    [n_rec, n_frames, S] (int64 atoms per species, element-list order)."""
    raw = np.asarray(raw, dtype=float)
    n_rec = raw.shape[0]
    return dict(trial=first_trial + every * np.arange(1, n_rec + 1, dtype=np.int64),
                energy=raw[..., 0].copy(), accepted=np.rint(raw[..., 1]).astype(np.int64),
                trials=np.rint(raw[..., 2]).astype(np.int64), composition=np.rint(raw[..., 3:]).astype(np.int64))


class MonteCarlo(Driver):
    KIND, WHO = "mc", WHO

    def __init__(self, calculator, atoms_or_list, temperature_K, mode="swap", chemical_potentials=None, swappable=None, seed=0,
                 device=None):
        """``temperature_K``: a scalar or one value per frame.  ``swappable``: boolean mask [sum N] over the concatenated
        frames; atoms outside it keep their species.  ``chemical_potentials``: see the module text."""
        # every argument is checked before the device is touched
        if mode not in MODES:
            raise ValueError(f"MonteCarlo: mode must be 'swap' or 'transmute', got {mode!r}")
        self.mode = mode
        self.seed = check_int(WHO, "seed", seed, 0, (1 << 64) - 1)
        self._list = isinstance(atoms_or_list, (list, tuple))
        self.frames = frames_of(WHO, atoms_or_list)
        self.calculator = calculator
        self.element_list = list(calculator.bspline_config.element_list)
        self.temperature_K = _temperatures(temperature_K, len(self.frames))
        self.chemical_potentials = _chemical_potentials(mode, chemical_potentials, self.element_list)
        self._batch = _lib.FrameBatch(self.frames)
        if not np.all(np.isfinite(self._batch.pos)):
            raise ValueError("MonteCarlo: positions must be finite")
        if not np.all(np.isfinite(self._batch.cells)):
            raise ValueError("MonteCarlo: cells must be finite")
        known = {atomic_numbers[e] for e in self.element_list}
        foreign = sorted({int(q) for q in self._batch.z} - known)
        if foreign:
            raise ValueError("MonteCarlo: the frames hold elements outside the model: "
                             + ", ".join(chemical_symbols[q] if 0 < q < len(chemical_symbols) else str(q) for q in foreign))
        self.swappable = check_mask(WHO, "swappable", swappable, self._batch.n_atoms)
        self.n_atoms = np.diff(self._batch.offsets).astype(np.int64)
        self.trial = 0
        self._create(calculator, device, [_lib._p(self._batch.pos), _lib._p(self._batch.z), _lib._p(self.swappable)])

    # ---- state ------------------------------------------------------------------------------------------------------------
    def _state(self, *which):
        nf, n = self._batch.n_frames, self._batch.n_atoms
        shapes = dict(z=((n,), np.int32), energies=((nf,), float), accepted=((nf,), np.int64), trials=((nf,), np.int64),
                      status=((nf,), np.int32))
        return self._fetch(shapes, which)

    @property
    def numbers(self):
        """[sum N] the current atomic numbers, frames concatenated."""
        return self._state("z")["z"]

    @property
    def acceptance(self):
        """[n_frames] accepted / counted trials so far (NaN before the first trial)."""
        s = self._state("accepted", "trials")
        return np.where(s["trials"] > 0, s["accepted"] / np.maximum(s["trials"], 1), np.nan)

    @property
    def status(self):
        """Per frame "running" or "nonfinite" (a non-finite energy difference froze the frame)."""
        return [STATUS[int(x)] for x in self._state("status")["status"]]

    def get_potential_energies(self):
        """[n_frames] eV: the running energies (the evaluator's at creation plus every accepted difference)."""
        return self._state("energies")["energies"]

    def get_atoms(self):
        """The frames with their current species: a list when a list was given, else one object."""
        from uf3_amd.data.atoms import Atoms
        z, off = self.numbers, self._batch.offsets
        out = [Atoms(numbers=z[off[k]:off[k + 1]].astype(np.int64), positions=self._batch.pos[off[k]:off[k + 1]].copy(),
                     cell=self._batch.cells[k].copy(), pbc=a.get_pbc()) for k, a in enumerate(self.frames)]
        return out if self._list else out[0]

    def set_positions(self, positions):
        """[N, 3] Angstrom (frames concatenated): the neighbour table is rebuilt, the species stay."""
        p = np.ascontiguousarray(np.asarray(positions, dtype=float))
        if p.shape != (self._batch.n_atoms, 3):
            raise ValueError(f"MonteCarlo: positions must be [{self._batch.n_atoms}, 3], got {np.shape(positions)}")
        if not np.all(np.isfinite(p)):
            raise ValueError("MonteCarlo: positions must be finite")
        self.ctx.check(self.ctx.lib.uf3_mc_set_positions(self._live(), _lib._p(p)))
        np.copyto(self._batch.pos, p)

    def delta_energy(self, frame, i, j_or_symbol):
        """Energy difference(s) of proposed moves on the current species, nothing applied.  ``frame``, ``i``: scalars or equal
        length sequences (frame index, atom index within the frame).  ``j_or_symbol``: in swap mode the second atom within the
        frame, in transmute mode the new element (symbol or atomic number).  Returns a float for scalars, else an array."""
        scalar = np.ndim(frame) == 0 and np.ndim(i) == 0
        f = np.atleast_1d(np.asarray(frame)).reshape(-1)
        a = np.atleast_1d(np.asarray(i)).reshape(-1)
        second = list(j_or_symbol) if isinstance(j_or_symbol, (list, tuple, np.ndarray)) else [j_or_symbol] * max(len(f), len(a))
        if not (len(f) == len(a) == len(second)):
            raise ValueError("MonteCarlo: delta_energy needs as many frames as atoms as partners")
        for name, arr in (("frame", f), ("i", a)):
            if arr.dtype.kind not in "iu":
                raise ValueError(f"MonteCarlo: delta_energy: {name} must be integer")
        if np.any(f < 0) or np.any(f >= self._batch.n_frames):
            raise ValueError("MonteCarlo: delta_energy: frame outside the batch")
        if np.any(a < 0) or np.any(a >= self.n_atoms[f]):
            raise ValueError("MonteCarlo: delta_energy: atom i outside its frame")
        if self.mode == "swap":
            s = np.asarray(second)
            if s.dtype.kind not in "iu":
                raise ValueError("MonteCarlo: delta_energy: in swap mode j must be an atom index")
            if np.any(s < 0) or np.any(s >= self.n_atoms[f]):
                raise ValueError("MonteCarlo: delta_energy: atom j outside its frame")
        else:
            s = np.array([atomic_numbers[self.element_list[_species_index(self.element_list, q, "delta_energy")]] for q in second])
        f, a, s = (np.ascontiguousarray(x, dtype=np.int32) for x in (f, a, s))
        out = np.empty(len(f))
        self.ctx.check(self.ctx.lib.uf3_mc_delta(self._live(), len(f), _lib._p(f), _lib._p(a), _lib._p(s), MODES[self.mode],
                                                 _lib._p(out)))
        return float(out[0]) if scalar else out

    # ---- sampling ---------------------------------------------------------------------------------------------------------
    def run(self, n_trials, record_every=0):
        """``n_trials`` trials of every frame.  Returns ``energy`` [n_frames] (running energies, eV), ``accepted`` and
        ``trials`` [n_frames] (totals so far; null trials -- like species, the same atom twice, an atom outside ``swappable``
        -- are counted and never accepted), ``composition`` [n_frames, S] (atoms per species, element-list order), ``status``;
        with ``record_every`` > 0 also ``records`` (``run_records``) after every ``record_every``-th trial of this run."""
        n_trials = check_int(WHO, "n_trials", n_trials)
        every = check_int(WHO, "record_every", record_every)
        temps = _temperatures(self.temperature_K, self._batch.n_frames)
        mu = self.chemical_potentials
        if (self.mode == "transmute") != (mu is not None):
            raise ValueError("MonteCarlo: chemical_potentials belong to mode='transmute', and that mode needs them")
        seed = check_int(WHO, "seed", self.seed, 0, (1 << 64) - 1)
        handle = self._live()
        n_rec = n_trials // every if every else 0
        raw = np.zeros((n_rec, self._batch.n_frames, 3 + len(self.element_list)))
        first = self.trial
        self.ctx.check(self.ctx.lib.uf3_mc_run(handle, n_trials, MODES[self.mode], _lib._p(temps), _lib._p(mu), seed, every,
                                               _lib._p(raw) if n_rec else None))
        self.trial += n_trials
        s = self._state("z", "energies", "accepted", "trials", "status")
        out = dict(energy=s["energies"], accepted=s["accepted"], trials=s["trials"],
                   composition=composition(s["z"], self._batch.offsets, self.element_list),
                   status=[STATUS[int(x)] for x in s["status"]])
        if n_rec:
            out["records"] = run_records(raw, first, every)
        return out


def composition(numbers_, offsets, element_list):
    """[n_frames, S] atoms of each species of ``element_list`` in the frames ``offsets`` cuts out of ``numbers_``."""
    zs = [atomic_numbers[e] for e in element_list]
    z = np.asarray(numbers_)
    return np.array([[int(np.sum(z[lo:hi] == q)) for q in zs] for lo, hi in zip(offsets[:-1], offsets[1:])], dtype=np.int64)


def short_range_order(atoms, r_shell, r_inner=0.0):
    """Warren-Cowley parameters of one frame over the neighbours at distances ``r_inner < d <= r_shell`` (every periodic
    image within reach counts on its own): ``alpha[a][b] = 1 - P(b | a) / c_b``, P(b | a) the fraction of b among the
    neighbours of the a atoms and c_b the concentration of b.  0: random, negative: a and b attract, positive: they avoid each
    other (B2 order on the first shell: -1).  Returns ``{"species": [Z ...] ascending, "alpha": [S, S], "neighbours": [S, S]
    counts}``; a row without neighbours is NaN.  Host NumPy."""
    r_shell, r_inner = float(r_shell), float(r_inner)
    if not (np.isfinite(r_shell) and r_shell > 0) or not (0 <= r_inner < r_shell):
        raise ValueError(f"short_range_order: need 0 <= r_inner < r_shell, got {r_inner!r}, {r_shell!r}")
    z = np.asarray(atoms.get_atomic_numbers(), dtype=np.int64).reshape(-1)
    pos = np.asarray(atoms.get_positions(), dtype=float).reshape(-1, 3)
    cell = np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)
    pbc = np.asarray(atoms.get_pbc() if hasattr(atoms, "get_pbc") else atoms.pbc, dtype=bool).reshape(3)
    if len(z) < 1:
        raise ValueError("short_range_order: the frame has no atoms")
    # images per axis: enough that every neighbour within r_shell of an atom ANYWHERE (unwrapped positions included) is met
    reach = np.zeros(3, dtype=int)
    if pbc.any():
        if abs(np.linalg.det(np.where(pbc[:, None], cell, np.eye(3)))) < 1e-12:
            raise ValueError("short_range_order: the cell is singular along a periodic direction")
        eff = np.where(pbc[:, None], cell, np.eye(3))
        frac = pos @ np.linalg.inv(eff)
        spread = frac.max(0) - frac.min(0)
        heights = abs(np.linalg.det(eff)) / np.linalg.norm(np.cross(eff[[1, 2, 0]], eff[[2, 0, 1]]), axis=1)
        reach = np.where(pbc, np.ceil(r_shell / heights + spread).astype(int), 0)
    species = np.unique(z)
    idx = np.searchsorted(species, z)
    counts = np.zeros((len(species), len(species)), dtype=np.int64)
    for s0 in range(-reach[0], reach[0] + 1):
        for s1 in range(-reach[1], reach[1] + 1):
            for s2 in range(-reach[2], reach[2] + 1):
                off = s0 * cell[0] + s1 * cell[1] + s2 * cell[2]
                d = np.linalg.norm(pos[None, :, :] + off - pos[:, None, :], axis=2)
                hit = (d > r_inner) & (d <= r_shell)
                if s0 == 0 and s1 == 0 and s2 == 0:
                    hit &= ~np.eye(len(z), dtype=bool)
                np.add.at(counts, (idx[:, None].repeat(len(z), 1)[hit], idx[None, :].repeat(len(z), 0)[hit]), 1)
    conc = np.array([np.mean(z == q) for q in species])
    total = counts.sum(1, keepdims=True).astype(float)
    with np.errstate(invalid="ignore", divide="ignore"):
        alpha = 1.0 - (counts / total) / conc[None, :]
    alpha[total[:, 0] == 0] = np.nan
    return dict(species=[int(q) for q in species], alpha=alpha, neighbours=counts)
