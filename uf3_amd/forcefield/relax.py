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
import numpy as np

from uf3_amd import _lib
from uf3_amd.forcefield._driver import Driver, check_int, check_mask, check_real, frames_of

STATUS = {0: "running", 1: "converged", 2: "nonfinite"}
WHO = "Relaxation"


class Relaxation(Driver):
    """Batched FIRE relaxation of positions, optionally with the cell, on the device (module text above).

    Atoms outside the cell: positions are kept unwrapped and go to the evaluator as they are, and the evaluator takes the
    reference's finite image range around the positions as given (``include/uf3_hip.h``, above ``uf3_md_create``; DESIGN.md
    section 7).  An atom that leaves its cell during a relaxation loses the interactions that range no longer reaches from where it
    is: energies and forces are then ``evaluate_frames``' of the unwrapped positions, not the wrapped crystal's.  Start from
    wrapped frames, and wrap the positions again before continuing a relaxation that moved atoms across a cell face."""
    KIND, WHO = "relax", WHO

    def __init__(self, calc, atoms_or_list, relax_cell=False, fixed=None, skin=0.5, device=None):
        """``fixed``: boolean mask [sum N] over the concatenated frames (ASE's FixAtoms): those atoms feel no force and never
        move; not together with ``relax_cell``.  ``skin`` (Angstrom): the evaluator's neighbour-list skin in positions-only
        runs (cell runs use 0)."""
        # every argument is checked before the device is touched
        if not isinstance(relax_cell, (bool, np.bool_)):
            raise ValueError(f"Relaxation: relax_cell must be True or False, got {relax_cell!r}")
        self.relax_cell = bool(relax_cell)
        self.skin = check_real(WHO, "skin", skin, hi=4.0)
        self._list = isinstance(atoms_or_list, (list, tuple))
        self.frames = frames_of(WHO, atoms_or_list)
        self.calculator = calc
        self._batch = _lib.FrameBatch(self.frames)
        if not np.all(np.isfinite(self._batch.pos)):
            raise ValueError("Relaxation: positions must be finite")
        if not np.all(np.isfinite(self._batch.cells)):
            raise ValueError("Relaxation: cells must be finite")
        self.fixed = check_mask(WHO, "fixed", fixed, self._batch.n_atoms)
        if self.fixed is not None and self.relax_cell:
            raise ValueError("Relaxation: fixed atoms together with relax_cell are not supported")
        self._create(calc, device, [_lib._p(self._batch.pos), _lib._p(self._batch.z), _lib._p(self.fixed)], [int(self.relax_cell)])

    # ---- state ------------------------------------------------------------------------------------------------------------
    def _state(self, *which):
        nf, n = self._batch.n_frames, self._batch.n_atoms
        shapes = dict(pos=((n, 3), float), cells=((nf, 3, 3), float), forces=((n, 3), float), energies=((nf,), float),
                      status=((nf,), np.int32), steps=((nf,), np.int64), fmax=((nf,), float))
        return self._fetch(shapes, which)

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
        max_steps = check_int(WHO, "max_steps", max_steps)
        fmax = check_real(WHO, "fmax", fmax, strict=True)
        dt = check_real(WHO, "dt", dt, strict=True)
        dt_max = check_real(WHO, "dt_max", dt_max, strict=True)
        maxstep = check_real(WHO, "maxstep", maxstep, strict=True)
        check_every = check_int(WHO, "check_every", check_every, 1)
        record_every = check_int(WHO, "record_every", record_every)
        skin = check_real(WHO, "skin", self.skin, hi=4.0)
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
