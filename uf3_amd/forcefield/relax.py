"""
``Relaxation``: FIRE relaxation of a batch of frames on the device (``uf3_relax_*`` in ``libuf3hip.so``).  Positions, forces
and every frame's optimiser state stay in HBM; each step is one evaluator call (``UFCalculator``'s model, its MD route with a
neighbour-list skin) and three small kernels.  Every frame is its own optimiser: it converges and freezes on its own, and its
trajectory does not depend on the batch around it.

FIRE follows ASE's formulation (N_min 5, f_inc 1.1, f_dec 0.5, alpha_start 0.1, f_alpha 0.99; mass-free; the first step keeps
``dt``; ``maxstep`` bounds the norm of a frame's whole step).  A frame has converged when every atom's |F_i| < ``fmax`` (ASE's
criterion).  With ``relax_cell`` the frames periodic along all three axes also relax their cell in ``UFCalculator.relax_fmax``'s
generalised coordinates (ASE's UnitCellFilter with cell_factor = n): x = q D, cell = cell0 D, cell coordinates n D, force on them
-D^-T W / n (W = dE/d(strain)); such a frame has also converged only when every row of D^-T W / n is below ``fmax``.  Non-finite
forces freeze a frame with status ``"nonfinite"``.

    with Relaxation(calc, frames, relax_cell=True) as rel:
        out = rel.run(500, fmax=1e-3)          # out["converged"], out["steps"], out["energy"], out["fmax"] per frame
        relaxed = rel.get_atoms()

``run`` may be called again: the FIRE state carries over, and ``run(a); run(b)`` follows ``run(a + b)``.  Positions are kept
unwrapped.  Cell runs wait for the device on every step (the evaluator reads the cells on the host) and rebuild their
neighbour lists every step; positions-only runs look at the device every ``check_every`` steps.
"""
import ctypes as C
import numbers
import os

import numpy as np

from uf3_amd import _lib

STATUS = {0: "running", 1: "converged", 2: "nonfinite"}


def _frames_of(atoms_or_list):
    frames = list(atoms_or_list) if isinstance(atoms_or_list, (list, tuple)) else [atoms_or_list]
    if not frames:
        raise ValueError("Relaxation: no frames")
    for k, a in enumerate(frames):
        if len(a) < 1:
            raise ValueError(f"Relaxation: frame {k} has no atoms")
    return frames


def _check_real(name, value, lo=0.0, strict=False, hi=None):
    try:
        x = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"Relaxation: {name} must be a number") from None
    if not np.isfinite(x) or (x <= lo if strict else x < lo) or (hi is not None and x > hi):
        bound = f"> {lo}" if strict else f">= {lo}"
        raise ValueError(f"Relaxation: {name} must be finite and {bound}" + (f" and <= {hi}" if hi is not None else "")
                         + f", got {value!r}")
    return x


def _check_int(name, value, lo=0):
    if isinstance(value, bool) or not isinstance(value, numbers.Integral) or value < lo:
        raise ValueError(f"Relaxation: {name} must be an integer >= {lo}, got {value!r}")
    return int(value)


def _fixed_mask(fixed, n_atoms):
    if fixed is None:
        return None
    m = np.asarray(fixed)
    if m.dtype != bool:
        raise ValueError("Relaxation: fixed must be a boolean mask over the concatenated atoms")
    m = m.reshape(-1)
    if m.size != n_atoms:
        raise ValueError(f"Relaxation: fixed holds {m.size} entries for {n_atoms} atoms")
    return np.ascontiguousarray(m.astype(np.uint8))


class Relaxation:
    def __init__(self, calc, atoms_or_list, relax_cell=False, fixed=None, skin=0.5, device=None):
        """``fixed``: boolean mask [sum N] over the concatenated frames (ASE's FixAtoms): those atoms feel no force and never
        move; not together with ``relax_cell``.  ``skin`` (Angstrom): the evaluator's neighbour-list skin in positions-only
        runs (cell runs use 0)."""
        self.handle = None
        # every argument is checked before the device is touched
        if not isinstance(relax_cell, (bool, np.bool_)):
            raise ValueError(f"Relaxation: relax_cell must be True or False, got {relax_cell!r}")
        self.relax_cell = bool(relax_cell)
        self.skin = _check_real("skin", skin, hi=4.0)
        self._list = isinstance(atoms_or_list, (list, tuple))
        self.frames = _frames_of(atoms_or_list)
        self.calculator = calc
        self._batch = _lib.FrameBatch(self.frames)
        if not np.all(np.isfinite(self._batch.pos)):
            raise ValueError("Relaxation: positions must be finite")
        if not np.all(np.isfinite(self._batch.cells)):
            raise ValueError("Relaxation: cells must be finite")
        self.fixed = _fixed_mask(fixed, self._batch.n_atoms)
        if self.fixed is not None and self.relax_cell:
            raise ValueError("Relaxation: fixed atoms together with relax_cell are not supported")
        self.ctx = _lib.get_context(calc.device if device is None else device)
        self._dbasis = _lib.device_basis(calc.bspline_config, self.ctx)
        self._pid = os.getpid()
        h = C.c_void_p()
        self.ctx.check(self.ctx.lib.uf3_relax_create(self._dbasis.handle, C.byref(self._batch.struct), _lib._p(self._batch.pos),
                                                     _lib._p(self._batch.z), _lib._p(self.fixed), _lib._p(calc._c1),
                                                     _lib._p(calc._c2), _lib._p(calc._c3), int(self.relax_cell), C.byref(h)))
        self.handle = h

    # ---- lifecycle --------------------------------------------------------------------------------------------------------
    def _live(self):
        if not self.handle:
            raise RuntimeError("Relaxation: the object is closed")
        return self.handle

    def close(self):
        if getattr(self, "handle", None):
            if os.getpid() == self._pid and self.ctx.handle:
                self.ctx.lib.uf3_relax_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- state ------------------------------------------------------------------------------------------------------------
    def _state(self, *which):
        nf, n = self._batch.n_frames, self._batch.n_atoms
        shapes = dict(pos=((n, 3), float), cells=((nf, 3, 3), float), forces=((n, 3), float), energies=((nf,), float),
                      status=((nf,), np.int32), steps=((nf,), np.int64), fmax=((nf,), float))
        out = {k: np.empty(*shapes[k]) for k in which}
        args = [_lib._p(out[k]) if k in out else None for k in shapes]
        self.ctx.check(self.ctx.lib.uf3_relax_get_state(self._live(), *args))
        return out

    def get_positions(self):
        """[N, 3] Angstrom, frames concatenated, unwrapped."""
        return self._state("pos")["pos"]

    def get_cells(self):
        """[n_frames, 3, 3] Angstrom (rows = lattice vectors)."""
        return self._state("cells")["cells"]

    def get_forces(self):
        """[N, 3] eV / Angstrom (Cartesian) at the current positions."""
        return self._state("forces")["forces"]

    def get_potential_energies(self):
        """[n_frames] eV at the current positions."""
        return self._state("energies")["energies"]

    def get_atoms(self):
        """The frames at the current positions and cells: a list when a list was given, else one object."""
        from uf3_amd.data.atoms import Atoms
        s = self._state("pos", "cells")
        off = self._batch.offsets
        out = [Atoms(numbers=a.get_atomic_numbers(), positions=s["pos"][off[k]:off[k + 1]], cell=s["cells"][k], pbc=a.get_pbc())
               for k, a in enumerate(self.frames)]
        return out if self._list else out[0]

    # ---- optimisation -----------------------------------------------------------------------------------------------------
    def run(self, max_steps, fmax=0.05, dt=0.1, dt_max=1.0, maxstep=0.2, check_every=10, record_every=0):
        """Up to ``max_steps`` FIRE steps of every frame still running (evaluations 0 .. max_steps, ASE's ``run(fmax, steps)``).
        Returns per frame: ``converged`` (bool), ``status`` ("running" | "converged" | "nonfinite"), ``steps`` (moves made in
        all runs so far), ``energy`` and ``fmax`` (the criterion) at the last evaluation; with ``record_every`` > 0 also
        ``records``: ``iteration`` [n_rec] and ``energy`` / ``fmax`` [n_rec, n_frames] of evaluations 0, record_every, ...
        (after every frame stopped, the final values repeat)."""
        max_steps = _check_int("max_steps", max_steps)
        fmax = _check_real("fmax", fmax, strict=True)
        dt = _check_real("dt", dt, strict=True)
        dt_max = _check_real("dt_max", dt_max, strict=True)
        maxstep = _check_real("maxstep", maxstep, strict=True)
        check_every = _check_int("check_every", check_every, 1)
        record_every = _check_int("record_every", record_every)
        skin = _check_real("skin", self.skin, hi=4.0)
        handle = self._live()
        n_rec = max_steps // record_every + 1 if record_every else 0
        raw = np.zeros((n_rec, self._batch.n_frames, 2))
        self.ctx.check(self.ctx.lib.uf3_relax_run(handle, max_steps, fmax, dt, dt_max, maxstep, skin, check_every, record_every,
                                                  _lib._p(raw) if n_rec else None))
        s = self._state("status", "steps", "fmax", "energies")     # (the last evaluation's: nothing has moved since)
        out = dict(converged=s["status"] == 1, status=[STATUS[int(x)] for x in s["status"]], steps=s["steps"],
                   energy=s["energies"], fmax=s["fmax"])
        if n_rec:
            out["records"] = dict(iteration=record_every * np.arange(n_rec, dtype=np.int64), energy=raw[..., 0].copy(),
                                  fmax=raw[..., 1].copy())
        return out
