"""Skewed and turned cells for the four drivers that own their positions and cells between evaluator calls (MD, NPT,
relaxation, NEB): the frames, reference trajectories whose energies, forces and strain derivatives come from the oracle alone
(the NumPy restatements _md_ref, _npt_ref, _relax_ref, _neb_ref driven by ``oracle.evaluate(..., virial=True)``: no reference
trajectory touches the device), and the mappings that carry a description's trajectory back to the original's.  For
tests/test_driver_cells_host.py (what the references alone prove) and tests/test_gpu_driver_cells.py (the kernels).

Which description is covariant for which driver (``admissible``):
- Langevin and piston noise is drawn per atom index in Cartesian axes: Langevin runs compare only descriptions that keep the
  atom order and the axes (a pure unimodular ``U``);
- supercells are covariant for NVE only: the piston mass, the cell coordinates n D and FIRE's trust radius (a norm over all
  degrees of freedom of a frame) depend on the atom count;
- everything else (rotations, reflections, permutations, rigid shifts, ``U``) is covariant for NVE, NPH, FIRE and NEB.  FIRE's
  convergence criterion takes row norms of G and is not rotation-invariant (ASE's convention), so covariance runs use an
  ``fmax`` nothing reaches and a fixed number of steps."""
import functools
import os

import numpy as np

from oracle import oracle as O
from uf3_amd import synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import md
from uf3_amd.regression import least_squares as ls
import _md_ref as MR
import _neb_ref as NR
import _npt_ref as PR
import _relax_ref as R
import test_redescribed_host as RH
from _util import GOLDEN, SKEW_U, describe, rotation, wrap_positions, wrapped

ORIGINAL = RH.ORIGINAL
MASSES = {"W": 180.0, "Mo": 96.0, "Nb": 93.0}          # test values, not a periodic table (tests/test_gpu_md.py)
TURN = rotation([1, 2, 3], 0.7)
# three times the strain of D in test_relax_host.py::test_cell_force_matches_central_differences_of_the_energy (3 to 9 %, not
# symmetric).  dE/d(strain) is symmetric whatever the cell, so D leaves the symmetric matrices only through D^-T W, by the
# square of the strain, and a swap of D against its transpose moves the run by the cube: at that D itself (1 to 3 %)
# G = -D^-1 W / n moved positions and cell by 2.8e-7 A in 30 steps, at twice it by 1.7e-5, at three times by 8e-5 and
# g = F D by 4.5e-6.
SHEAR = np.eye(3) + 3.0 * (np.array([[1.01, 0.02, -0.01], [0.005, 0.99, 0.015], [-0.02, 0.01, 1.03]]) - np.eye(3))
# the rigid shifts equivalence_cases() gave its descriptions (a Description does not keep them; ``residual`` at step 0 shows
# in the host test that these are the ones)
SHIFTS = {("bcc_mow", "perm_rotation_shift"): [1.1, -0.4, 2.2], ("wire_mow", "perm_rotation_shift"): [2.0, 0.3, 0.1]}
NEVER = 1e-12                                           # an fmax that nothing reaches in 30 steps
# FIRE on the short runs: a trust radius of 0.02 A per step (over all degrees of freedom of a frame).  The seeded model is no
# physical one and at ASE's default of 0.2 A its atoms travel more than 1 A in 30 steps, out of the window of DESIGN.md section 7
# (by 1.25 A on the 16-atom cell), where descriptions of one crystal stop being equivalent: the oracle-driven restatement then
# differs by 1e-2 A between descriptions.  At 0.02 A every atom stays inside (tests/test_driver_cells_host.py prints the room).
FIRE_KW = dict(dt=0.1, dt_max=0.3, maxstep=0.02)
FIRE_KW_DEFAULT = dict(dt=0.1, dt_max=1.0, maxstep=0.2)
N_STEPS = 30                                            # every short run: MD, NPT, FIRE, NEB
# piston settings of test_gpu_npt.py's parity runs
NPT_KW = dict(p0=0.02, tau=1000.0)
MD_SEED, V_SEED = 9, 4

# (case, label) of every description the MD driver meets, each compared with its case's original
MD_DESCRIPTIONS = [("bcc_mow", "skew_821"), ("bcc_mow", "skew_351"), ("bcc_mow", "perm_rotation_shift"),
                   ("bcc_mow", "skew_751_reflection"), ("ternary", "skew_751"), ("slab_mow", "skew_in_plane_531"),
                   ("slab_mow", "supercell_211_rotation"), ("wire_mow", "perm_rotation_shift")]
# the parity cases the issue names, alone; MIXED: the batch that holds a skewed bulk, a turned slab and a wire
PARITY = [("bcc_mow", "skew_821"), ("bcc_mow", "skew_751_reflection")]
NPT_PARITY = PARITY + [("ternary", "skew_751")]
MIXED = [("bcc_mow", "skew_821"), ("slab_mow", "supercell_211_rotation"), ("wire_mow", "perm_rotation_shift")]
MIXED_FIRE = [("bcc_mow", "skew_751_reflection"), ("slab_mow", "skew_in_plane_531"), ("wire_mow", "perm_rotation_shift")]


W_UNARY = "w_unary"              # the sheared cell-relaxation start: bcc W under tests/golden/model_unary.json
A0_W = 3.17352                   # that model's lattice constant (tests/test_gpu_relax.py)


def model_case(case):
    """The model a frame of ``case`` is run with: one Mo/W model for bulk, slab and wire, so that they share a batch."""
    return case if case in ("ternary", W_UNARY) else "bcc_mow"


@functools.lru_cache(maxsize=None)
def model(case):
    """The model object of a case (one per process: device tables hang on its basis)."""
    m = model_case(case)
    return ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json")) if m == W_UNARY else RH.model(m)


@functools.lru_cache(maxsize=None)
def _oracle_model(case):
    mdl = model(case)
    return O.OracleBasis(mdl.bspline_config), np.asarray(mdl.coefficients, dtype=float)


def fire_kw(case):
    """FIRE's settings on the short runs: ASE's defaults under the W model, a small trust radius under the seeded ones."""
    return FIRE_KW_DEFAULT if model_case(case) == W_UNARY else FIRE_KW


def heights(cell):
    """Perpendicular heights of a cell (rows = lattice vectors): vol / |n_k|."""
    c = np.asarray(cell, float).reshape(3, 3)
    n = np.array([np.cross(c[1], c[2]), np.cross(c[2], c[0]), np.cross(c[0], c[1])])
    return abs(np.linalg.det(c)) / np.linalg.norm(n, axis=1)


def image_ratio(cell, r_cut):
    """r_cut / height per axis: its ceiling is the build's image range ``fac``."""
    return r_cut / heights(cell)


def r_cut(case):
    return float(model(case).bspline_config.r_cut)


class Pair:
    """An original frame, one description of it and what maps the description's results back."""

    def __init__(self, case, label, base, d, shift=None):
        self.case, self.label, self.base, self.d = case, label, base, d
        self.shift = np.zeros(3) if shift is None else np.asarray(shift, float)
        self.cell0 = np.asarray(base.get_cell(), float).reshape(3, 3)
        self.pbc = np.asarray(base.get_pbc(), bool)

    @property
    def atoms(self):
        return self.base if self.d is None else self.d.atoms

    @property
    def pure_u(self):
        d = self.d
        return d is None or (d.scale == 1 and np.array_equal(d.Q, np.eye(3)) and np.array_equal(d.src, np.arange(len(d.src)))
                             and not self.shift.any())

    def admissible(self, driver):
        """driver: nve, langevin, nph, npt (the Langevin piston), fire, neb"""
        if self.d is None:
            return True
        if driver in ("langevin", "npt"):
            return self.pure_u
        if driver == "nve":
            return True
        return self.d.scale == 1

    # ---- mappings: original's quantity -> the description's -------------------------------------------------------------
    def vectors(self, v):
        """velocities, forces, NEB forces"""
        return np.asarray(v) if self.d is None else self.d.forces(v)

    def strain(self, w):
        """strain derivatives and stress records (Voigt)"""
        return np.asarray(w) if self.d is None else self.d.virial(w)

    def energy(self, e):
        return e if self.d is None else self.d.energy(e)

    def deformation(self, D):
        """D' = Q D Q^T"""
        return np.asarray(D) if self.d is None else self.d.Q @ D @ self.d.Q.T

    def residual(self, x_desc, x_orig, cell_now=None):
        """What is left of x' Q - x[src] - c after the nearest integer combination of the original's CURRENT cell rows is
        taken out along the periodic axes, [n', 3]; c is the rigid shift carried along with the cell (scaled by s under a
        piston, times D under a cell relaxation: c cell0^-1 cell_now)."""
        if self.d is None:
            return np.asarray(x_desc) - np.asarray(x_orig)
        cell = self.cell0 if cell_now is None else np.asarray(cell_now, float).reshape(3, 3)
        c = self.shift @ np.linalg.inv(self.cell0) @ cell
        diff = np.asarray(x_desc) @ self.d.Q - np.asarray(x_orig)[self.d.src] - c
        frac = diff @ np.linalg.inv(cell)
        frac[:, self.pbc] -= np.rint(frac[:, self.pbc])
        return frac @ cell


@functools.lru_cache(maxsize=None)
def pair(case, label):
    base, descs = RH.CASES[case]
    if label == ORIGINAL:
        return Pair(case, label, base, None)
    return Pair(case, label, base, next(d for d in descs if d.label == label), SHIFTS.get((case, label)))


@functools.lru_cache(maxsize=None)
def sheared(label):
    """The cell-relaxation start that is neither symmetric nor diagonal: a 16-atom bcc W cell at the W model's lattice constant
    (rattled by 0.03 A), deformed homogeneously by SHEAR (cell and positions alike: ``original``), then described by skew_821
    and turned (``sheared_turned``).  Under the W model the atoms stay near their sites and FIRE's trust radius goes to the
    cell: D travels 3 % in 30 steps and leaves the symmetric matrices by the square of that, which is what the swaps of
    tests/test_driver_cells_host.py (d) need; the seeded Mo/W models push their atoms out of the window long before."""
    bcc = wrapped(synthetic.lattice_frame("bcc", (2, 2, 2), A0_W, [74], seed=81, rattle=0.03, strain=0.0))
    cell = np.asarray(bcc.get_cell(), float) @ SHEAR
    base = wrapped(Atoms(numbers=bcc.get_atomic_numbers(), positions=bcc.get_positions() @ SHEAR, cell=cell, pbc=True))
    if label == ORIGINAL:
        return Pair(W_UNARY, "sheared", base, None)
    assert label == "sheared_turned"
    return Pair(W_UNARY, label, base, describe(base, label, U=SKEW_U["skew_821"], Q=TURN))


def get_pair(case, label):
    return sheared(ORIGINAL if label == "sheared" else label) if label in ("sheared", "sheared_turned") else pair(case, label)


# ---- NPT frames whose image range changes inside a short run ------------------------------------------------------------------
U_110 = [[1, 0, 0], [1, 1, 0], [0, 1, 1]]
# name -> U, lattice constant, the pressure (eV/A^3) that crosses and one that does not.  With r_cut = 5.5 the 3 x 3 x 3 Mo/W
# cell (synthetic.lattice_frame, seed 84, no strain) has r_cut / height on axis 0 of 4.983 (skew_821, a = 3.165: 0.35 % of
# compression take fac from 5 to 6), 0.992 (U_110, a = 3.2: 0.8 % take it from 1 to 2) and 4.020 (skew_751, a = 3.225: 0.5 % of
# expansion take it from 5 to 4; at a = 3.165 the ratio is 4.096 and the 2.4 % it needs put axis 1, at 2.95, across 3 first).
# The seeded model is under pressure of its own: at P = 0 the cells shrink by 0.8 to 1.1 % in 40 steps, so the runs that must
# stay on their side of the crossing pull (skew_821, U_110) or hold (skew_751) accordingly.  The host test prints the ratios
# and asserts the crossings.
CROSSINGS = {"skew_821_5to6": dict(U=SKEW_U["skew_821"], a=3.165, p_cross=0.05, p_stay=-0.05),
             "u110_1to2": dict(U=U_110, a=3.2, p_cross=0.05, p_stay=-0.05),
             "skew_751_5to4": dict(U=SKEW_U["skew_751"], a=3.225, p_cross=-0.06, p_stay=0.0)}
CROSS_STEPS = 40
CROSS_KW = dict(tau=1000.0, skin=0.2)           # test_a_compression_that_uses_up_the_skin_rebuilds_and_still_matches


@functools.lru_cache(maxsize=None)
def crossing(name):
    """The frame re-described by U and then moved rigidly to where its atoms are farthest from the cell's faces.  Next to a
    crossing r_cut / h is an integer, the window of fractional width fac + 1 - r_cut / h is the cell itself, and an atom at a
    face would leave it with its first move; the layers of the skewed cell leave room between them, and the shift (the best of
    4000 seeded candidates) puts the faces there."""
    spec = CROSSINGS[name]
    base = wrapped(synthetic.lattice_frame("bcc", (3, 3, 3), spec["a"], [42, 74], seed=84, strain=0.0))
    d = describe(base, name, U=spec["U"])
    cell = np.asarray(d.atoms.get_cell(), float)
    frac, h = d.atoms.get_positions() @ np.linalg.inv(cell), heights(cell)
    best, room = None, -1.0
    for t in np.random.default_rng(0).random((4000, 3)):
        f = (frac + t) % 1.0
        r = float((np.minimum(f, 1.0 - f) * h).min())
        if r > room:
            best, room = f, r
    d.atoms = Atoms(numbers=d.atoms.get_atomic_numbers(), positions=best @ cell, cell=cell, pbc=True)
    return Pair("bcc_mow", name, base, d)


# ---- the oracle as the drivers' evaluator ------------------------------------------------------------------------------------------
class OracleFrames:
    """Energies [nf], forces [N, 3] and dE/d(strain) [nf, 6] of a batch of frames from the oracle, at given positions and cells;
    keeps every (positions, cells) it was asked about (``trace``) for the window check."""

    def __init__(self, case, frames, recell=None):
        """``recell``: per frame None or a matrix M.  The oracle then sees that frame in the equivalent cell M @ cell, every
        atom folded into it.  For the 54-atom crossing frames, M = U^-1: in the thin skewed cell itself the oracle's image range
        no longer holds the third atom of every ghost-centred triplet and its forces lose those terms (DESIGN.md section 7:
        they differ from minus the gradient of its own energy by 3.0e-2 eV/A under skew_821 and 1.1e-2 under skew_751, which
        tests/test_driver_cells_host.py asserts), while in the 9.5 A cubic cell they are the gradient.  Energies and strain
        derivatives are the same in both cells."""
        self.ob, self.c = _oracle_model(case)
        self.recell = recell
        self.frames = list(frames)
        self.off = np.cumsum([0] + [len(a) for a in self.frames])
        self.cells0 = np.array([np.asarray(a.get_cell(), float).reshape(3, 3) for a in self.frames])
        self.trace = []

    def __call__(self, x, cells=None):
        cells = self.cells0 if cells is None else np.asarray(cells, float).reshape(-1, 3, 3)
        self.trace.append((np.array(x, float), np.array(cells, float)))
        es, fs, ws = [], [], []
        for k, a in enumerate(self.frames):
            pos, cell = x[self.off[k]:self.off[k + 1]], cells[k]
            if self.recell is not None and self.recell[k] is not None:
                cell = np.asarray(self.recell[k], float) @ cell
                pos = wrap_positions(cell, pos, a.get_pbc())
            moved = Atoms(numbers=a.get_atomic_numbers(), positions=pos, cell=cell, pbc=a.get_pbc())
            e, f, w = O.evaluate(self.ob, moved, self.c, forces=True, virial=True)
            es.append(e); fs.append(f); ws.append(w)
        return np.array(es), np.concatenate(fs), np.array(ws)

    # one callback per restatement
    def md(self):
        return lambda x: self(x)[:2]                                           # _md_ref.run: forces_of(x)

    def npt(self):
        def evaluate(x, s):                                                    # _npt_ref.run: evaluate(x, s)
            e, f, w = self(x, self.cells0 * np.asarray(s)[:, None, None])
            return e, f, w[:, :3].sum(1)
        return evaluate

    def relax(self):
        return lambda x, cells: self(x, cells)                                 # _relax_ref.Fire: evaluate(x, cells)

    def neb(self):
        return lambda x: self(x)[:2]                                           # _neb_ref.Band: evaluate(x)


def window_room(trace, frames, rc):
    """The smallest distance (Angstrom, along the axis' normal) by which any atom stays inside the window of fractional width
    fac + 1 - r_cut / h around its CURRENT cell, over every evaluation of a reference run; negative:
    an atom left it."""
    off = np.cumsum([0] + [len(a) for a in frames])
    room = np.inf
    for x, cells in trace:
        for k, a in enumerate(frames):
            per = np.asarray(a.get_pbc(), bool)
            if not per.any():
                continue
            h = heights(cells[k])
            w = np.ceil(rc / h) + 1.0 - rc / h
            frac = x[off[k]:off[k + 1]] @ np.linalg.inv(cells[k])
            r = np.minimum(frac - (0.5 - 0.5 * w), (0.5 + 0.5 * w) - frac) * h
            room = min(room, float(r[:, per].min()))
    return room


def masses_of(frames):
    return md.resolve_masses(list(frames), MASSES)


@functools.lru_cache(maxsize=None)
def _velocities0(case, label):
    base = get_pair(case, label).base
    v = MR.init_velocities(masses_of([base]), np.array([0, len(base)]), 300.0, V_SEED, 0)
    v.setflags(write=False)
    return v


def velocities(case, label):
    """Maxwell-Boltzmann velocities of the original (300 K, no net momentum), carried to the description."""
    return np.array(get_pair(case, label).vectors(_velocities0(case, label)))


def crossing_velocities(name):
    base = crossing(name).base
    return MR.init_velocities(masses_of([base]), np.array([0, len(base)]), 300.0, V_SEED, 0)


def _frozen(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


def batch_start(cases):
    """frames, x0, v0, masses, offsets of a batch of (case, label)"""
    frames = [get_pair(c, l).atoms for c, l in cases]
    off = np.cumsum([0] + [len(a) for a in frames])
    x0 = np.concatenate([a.get_positions() for a in frames])
    v0 = np.concatenate([velocities(c, l) for c, l in cases])
    return frames, x0, v0, masses_of(frames), off


# ---- reference runs (computed once per process, shared, never changed) ----------------------------------------------------------
@functools.lru_cache(maxsize=None)
def md_reference(cases, langevin, n_steps=N_STEPS):
    """``cases``: a tuple of (case, label), one batch.  x, v, e, f, w (dE/d(strain) at the end), room."""
    frames, x0, v0, m, off = batch_start(cases)
    ora = OracleFrames(cases[0][0], frames)
    t, g = (300.0, 0.05) if langevin else (0.0, 0.0)
    x, v, e, f = MR.run(x0, v0, m, ora.md(), n_steps, 1.0, t, g, MD_SEED)
    w = ora(x)[2]
    return _frozen(dict(x=x, v=v, e=np.asarray(e), f=f, w=w, room=window_room(ora.trace, frames, r_cut(cases[0][0])), x0=x0, v0=v0))


def npt_run(frames, x0, v0, case, n_steps, p0, tau, langevin, evaluate=None, recell=None):
    """One constant-pressure reference run; returns the result dict and the oracle object."""
    m, off = masses_of(frames), np.cumsum([0] + [len(a) for a in frames])
    ora = OracleFrames(case, frames, recell)
    P = PR.Pistons(off, np.abs(np.linalg.det(ora.cells0)), tau, 300.0)
    t, g, gp = (300.0, 0.05, 0.02) if langevin else (300.0, 0.0, 0.0)
    nf = len(frames)
    s_hist = []
    inner = ora.npt() if evaluate is None else evaluate(ora)

    x_hist = []

    def recording(x, s):
        s_hist.append(np.array(s))
        x_hist.append(np.array(x))
        return inner(x, s)
    x, v, s, ve, e, f = PR.run(x0, v0, m, P, np.ones(nf), np.zeros(nf), recording, n_steps, 1.0, p0, t if langevin else 0.0, g, gp,
                               MD_SEED)
    return dict(x=x, v=v, s=s, veps=ve, e=np.asarray(e), f=f, s_hist=np.array(s_hist), x_hist=np.array(x_hist), x0=x0, v0=v0), ora


@functools.lru_cache(maxsize=None)
def npt_reference(cases, langevin, n_steps=N_STEPS):
    frames, x0, v0, m, off = batch_start(cases)
    out, ora = npt_run(frames, x0, v0, cases[0][0], n_steps, NPT_KW["p0"], NPT_KW["tau"], langevin)
    out["room"] = window_room(ora.trace, frames, r_cut(cases[0][0]))
    return _frozen(out)


def edge_lengths(cell):
    """What a wrong list rule would take for the heights."""
    return np.linalg.norm(np.asarray(cell, float).reshape(3, 3), axis=1)


def list_rule(x_hist, s_hist, cell0, rc, skin, heights_of=heights, image_rule=True):
    """NumPy restatement of the list test of a constant-pressure run of ONE frame (uf3_npt.h: k_npt_frame's limits and
    k_npt_move's displacement test; uf3_hip.hip: what the evaluator does with the two status words), replayed on a trajectory:
    ``x_hist`` [n + 1, N, 3] and ``s_hist`` [n + 1] at every force evaluation, the first at the start.

    The lists are built at the first evaluation.  After the move of step k the reference positions of the lists are scaled
    with the cell, lim = (s / s_build (skin + r_cut) - r_cut) / 2, and the lists are void when an atom is farther than lim
    from its reference position, or when r_cut / (s height) has left (fb - 1, fb) on an axis, fb = ceil(r_cut / (s_build
    height)) the build's image range: the step is evaluated again on new lists (``redone``).  An atom beyond 0.7 lim is the
    early warning: new lists in front of the next step's evaluation.  Returns builds, redone and the steps of both kinds."""
    h0 = heights_of(cell0)
    s_build, xref, s_prev = float(s_hist[0]), np.array(x_hist[0]), float(s_hist[0])
    builds, stale, void_steps, early_steps = 1, False, [], []
    for k in range(1, len(s_hist)):
        s, x = float(s_hist[k]), x_hist[k]
        xref = xref * (s / s_prev)
        s_prev = s
        lim = 0.5 * (s / s_build * (skin + rc) - rc) * (1.0 - 1e-9)
        ok = lim > 0.0
        if image_rule:
            fb, now = np.ceil(rc / (s_build * h0)), rc / (s * h0)
            ok = ok and bool(np.all((now > fb - 1.0 + 1e-9) & (now < fb - 1e-9)))
        moved = ((x - xref) ** 2).sum(1).max()
        if stale:                                   # the early warning of the step before: lists of this step's positions
            builds, stale, s_build, xref = builds + 1, False, s, np.array(x)
            early_steps.append(k)
        elif not ok or not moved <= lim * lim:
            builds, s_build, xref = builds + 1, s, np.array(x)
            void_steps.append(k)
        elif not moved <= 0.49 * lim * lim:
            stale = True
    return dict(builds=builds, redone=len(void_steps), void_steps=void_steps, early_steps=early_steps)


def crossing_recell(name):
    """U^-1: the matrix that takes the crossing frame's cell back to the cubic one (OracleFrames: recell)."""
    P = crossing(name)
    return P.cell0 @ np.linalg.inv(np.asarray(P.atoms.get_cell(), float))


@functools.lru_cache(maxsize=None)
def crossing_reference(name, cross=True):
    P = crossing(name)
    spec = CROSSINGS[name]
    out, ora = npt_run([P.atoms], P.atoms.get_positions(), crossing_velocities(name), "bcc_mow", CROSS_STEPS,
                       spec["p_cross"] if cross else spec["p_stay"], CROSS_KW["tau"], False, recell=[crossing_recell(name)])
    out["room"] = window_room(ora.trace, [P.atoms], r_cut("bcc_mow"))
    out["ratio0"] = image_ratio(P.atoms.get_cell(), r_cut("bcc_mow"))
    for key, kw in (("lists", {}), ("lists_edge_lengths", dict(heights_of=edge_lengths)), ("lists_no_image_rule", dict(image_rule=False))):
        out[key] = list_rule(out["x_hist"], out["s_hist"][:, 0], P.atoms.get_cell(), r_cut("bcc_mow"), CROSS_KW["skin"], **kw)
    return _frozen(out)


def fire(cases, relax_cell, evaluate=None, fire_class=R.Fire):
    frames = [get_pair(c, l).atoms for c, l in cases]
    ora = OracleFrames(cases[0][0], frames)
    x0 = np.concatenate([a.get_positions() for a in frames])
    ref = fire_class(ora.relax() if evaluate is None else evaluate, x0, ora.cells0, [a.get_pbc() for a in frames], ora.off,
                     relax_cell=relax_cell)
    return ref, ora, frames


@functools.lru_cache(maxsize=None)
def fire_reference(cases, relax_cell, n_steps=N_STEPS):
    """30 FIRE steps at an fmax nothing reaches: x, cells, D, e, f at the last evaluation, the smallest normalised power."""
    ref, ora, frames = fire(cases, relax_cell)
    ref.run(n_steps, fmax=NEVER, **fire_kw(cases[0][0]))
    e, f, w = ref._forces
    return _frozen(dict(x=ref.x.copy(), cells=ref.cells.copy(), D=ref.D.copy(), e=ref.e_last.copy(), f=np.array(f), w=np.array(w),
                        status=ref.status.copy(), steps=ref.steps.copy(), power=np.array(ref.power),
                        room=window_room(ora.trace, frames, r_cut(cases[0][0]))))


# ---- NEB: test_gpu_neb.py's exchange of two unlike neighbours, on the 16-atom Mo/W cell ---------------------------------------
# NEB_TURN: the pair turns by 0.05 pi (9 degrees) along the band, not by pi.  The full exchange carries its two atoms 1.4 A off
# their sites, 0.7 A out of the window of DESIGN.md section 7 on the 16-atom cell (whose skew_351 description leaves 0.21 A of room),
# and there the oracle's energies of the two descriptions differ by 1.3e-3 eV; at 9 degrees every image stays 0.16 A inside.
NEB_IMAGES, NEB_SEED, NEB_SPRING, NEB_TURN = 6, 11, 0.2, 0.05


# _rattled and _exchange are tests/test_gpu_neb.py's, with ``turn`` added; the two must stay in step
# (tests/test_driver_cells_host.py: test_the_exchange_band_is_the_sibling_tests_construction compares them at turn = 1)
def _rattled(atoms, seed, rattle):
    x = atoms.get_positions() + np.random.default_rng(seed).normal(0, rattle, (len(atoms), 3))
    return Atoms(numbers=atoms.get_atomic_numbers(), positions=x, cell=atoms.get_cell(), pbc=atoms.get_pbc())


def _exchange(atoms, m, seed, rattle=(0.002, 0.005), turn=1.0):
    """tests/test_gpu_neb.py: _exchange (the pair turning about its centre, end points rattled independently), the pair
    turned by ``turn`` * pi in all."""
    x, z = atoms.get_positions(), atoms.get_atomic_numbers()
    d = np.linalg.norm(x[None] - x[:, None], axis=-1) + 1e3 * (z[None] == z[:, None])
    i, j = np.unravel_index(np.argmin(d), d.shape)
    mid, half = 0.5 * (x[i] + x[j]), 0.5 * (x[i] - x[j])
    axis = np.cross(half, [0.3, 0.5, 0.81])
    axis /= np.linalg.norm(axis)
    ends = [_rattled(atoms, seed, rattle[0]).get_positions(), _rattled(atoms, seed + 1000, rattle[1]).get_positions()]
    band = []
    for k in range(m):
        t = k / (m - 1)
        y = (1 - t) * ends[0] + t * ends[1]
        c, s_ = np.cos(np.pi * turn * t), np.sin(np.pi * turn * t)
        turned = half * c + np.cross(axis, half) * s_
        y[i] += mid + turned - x[i]
        y[j] += mid - turned - x[j]
        band.append(Atoms(numbers=z, positions=y, cell=atoms.get_cell(), pbc=atoms.get_pbc()))
    return band


@functools.lru_cache(maxsize=None)
def neb_band(label):
    """(Pair, [images]): the band built on the original cell, every image carried to the description by the same lattice
    translations, permutation and rotation as the frame itself (each image is described on its own and then moved by the
    lattice vectors that keep it next to image 0, so that differences between images are the original's, turned)."""
    base = RH.CASES["bcc_mow"][0]
    band0 = _exchange(base, NEB_IMAGES, NEB_SEED, turn=NEB_TURN)
    if label == ORIGINAL:
        return Pair("bcc_mow", label, base, None), band0
    assert label == "skew_351_turned"
    d = describe(base, label, U=SKEW_U["skew_351"], Q=TURN)
    P = Pair("bcc_mow", label, base, d)
    # base atom k sits at x_d Q = x_base + (lattice vector t_k): carry t_k, not the wrap of each image, along the band
    t = d.atoms.get_positions() @ d.Q - base.get_positions()[d.src]
    band = [Atoms(numbers=d.atoms.get_atomic_numbers(), positions=(a.get_positions()[d.src] + t) @ d.Q.T, cell=d.atoms.get_cell(),
                  pbc=True) for a in band0]
    return P, band


def neb_fixed(label):
    """The fixed-atom mask of the band (three atoms of the original, carried through ``src``), over all images."""
    P, band = neb_band(label)
    mask0 = np.zeros(len(P.base), bool)
    mask0[[2, 7, 12]] = True
    one = mask0 if P.d is None else mask0[P.d.src]
    return np.tile(one, len(band))


def neb(label, fixed=False, band_class=NR.Band):
    P, band = neb_band(label)
    ora = OracleFrames("bcc_mow", band)
    x0 = np.concatenate([a.get_positions() for a in band])
    ref = band_class(ora.neb(), x0, ora.off, np.array([0, len(band)]), spring=NEB_SPRING, fixed=neb_fixed(label) if fixed else None)
    return ref, ora, band


@functools.lru_cache(maxsize=None)
def neb_reference(label, climb, fixed=False, n_steps=N_STEPS):
    ref, ora, band = neb(label, fixed)
    ref.run(n_steps, fmax=NEVER, climb=climb, **FIRE_KW)
    return _frozen(dict(x=ref.x.copy(), e=ref.e_last.copy(), g=ref.g.copy(), f=np.array(ref._forces[1]), crit=ref.crit.copy(),
                        climbing=ref.climbing.copy(), status=ref.status.copy(), steps=ref.steps.copy(),
                        margins=np.array(ref.margins), power=np.array(ref.power),
                        room=window_room(ora.trace, band, r_cut("bcc_mow"))))
