"""NumPy restatement of the mean-squared-displacement record of ``uf3_md_run_msd`` (uf3_amd/csrc/uf3_md.h: k_md_msd_partial,
k_md_msd_frame), the direct formulas its host-side derivations are checked against, and the projectile run in which an atom
crosses cell faces (the references of tests/test_md_wrap_host.py and tests/test_gpu_md_wrap.py: the oracle alone, no device)."""
import functools

import numpy as np

import _driver_cells as DC
import _md_ref as MR
from uf3_amd.forcefield.md import ACC


def record(x, origin, masses, species, offsets, n_species, magnitudes=False):
    """[n_frames, 4 S + 4] of unwrapped positions ``x`` [N, 3]: per species sum |dr|^2, sum dx, sum dy, sum dz over its atoms,
    dr = x - origin; then sum m dr (3) and sum m over the frame.  ``species`` [N]: the species index of every atom.
    ``magnitudes``: the sums of the terms' absolute values instead, the scale a sum's rounding error is relative to (sum m dr
    of a run without net momentum is zero up to that rounding)."""
    dr = np.asarray(x, float) - np.asarray(origin, float)
    if magnitudes:
        dr = np.abs(dr)
    out = np.zeros((len(offsets) - 1, 4 * n_species + 4))
    for f, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
        d, m, s = dr[lo:hi], np.asarray(masses, float)[lo:hi], np.asarray(species)[lo:hi]
        for q in range(n_species):
            out[f, 4 * q] = (d[s == q] ** 2).sum()
            out[f, 4 * q + 1:4 * q + 4] = d[s == q].sum(0)
        out[f, 4 * n_species:4 * n_species + 3] = (m[:, None] * d).sum(0)
        out[f, 4 * n_species + 3] = m.sum()
    return out


def direct(x, origin, masses, species, offsets, n_species):
    """The quantities themselves, atom by atom: msd [nf, S] (NaN for a species the frame lacks), msd_all [nf], and both with
    the frame's mass-weighted centre-of-mass displacement taken out of every atom's displacement first."""
    dr = np.asarray(x, float) - np.asarray(origin, float)
    nf = len(offsets) - 1
    msd, com = np.full((nf, n_species), np.nan), np.full((nf, n_species), np.nan)
    msd_all, com_all = np.zeros(nf), np.zeros(nf)
    for f, (lo, hi) in enumerate(zip(offsets[:-1], offsets[1:])):
        d, m, s = dr[lo:hi], np.asarray(masses, float)[lo:hi], np.asarray(species)[lo:hi]
        rel = d - (m[:, None] * d).sum(0) / m.sum()
        msd_all[f], com_all[f] = (d ** 2).sum(1).mean(), (rel ** 2).sum(1).mean()
        for q in range(n_species):
            if (s == q).any():
                msd[f, q], com[f, q] = (d[s == q] ** 2).sum(1).mean(), (rel[s == q] ** 2).sum(1).mean()
    return msd, msd_all, com, com_all


def species_of(atoms_list, zs):
    """The species index (position in the ascending atomic numbers ``zs``) of every atom of the concatenated frames."""
    z = np.concatenate([np.asarray(a.get_atomic_numbers()) for a in atoms_list])
    return np.searchsorted(np.asarray(zs), z)


# ---- the projectile: one atom of the 16-atom Mo/W cell sent across cell faces ------------------------------------------------------
CASE = "bcc_mow"
ATOM = 3
DIRECTION = np.array([1.0, 0.3, 0.2])
# name -> extra speed of atom 3 (Angstrom / fs), steps
FLIGHTS = {"fast": (0.4, 40), "slow": (0.2, 30)}


def base():
    return DC.get_pair(CASE, DC.ORIGINAL).base


def start(name):
    """x0, v0, masses of a flight: the 300 K velocities of tests/_driver_cells.py, atom 3 given its extra velocity, the net
    momentum then removed."""
    a = base()
    m = DC.masses_of([a])
    v = np.array(MR.init_velocities(m, np.array([0, len(a)]), 300.0, DC.V_SEED, 0))
    v[ATOM] += FLIGHTS[name][0] * DIRECTION
    v -= (m[:, None] * v).sum(0) / m.sum()
    return np.array(a.get_positions(), float), v, m


@functools.lru_cache(maxsize=None)
def flight(name, rule, dx=0.0):
    """A reference run of ``_md_ref.run`` (NVE, 1 fs) driven by the oracle.  ``rule``: "unwrapped" evaluates the positions as
    they are (the rule of a ``wrap=False`` object), "wrapped" folds them into the cell in front of every evaluation.  ``dx``:
    the start positions moved by that much along x (the reference's sensitivity).  x, v, e, f at the end, every evaluation's
    positions ``x_hist`` [n + 1, N, 3] and the window room."""
    x0, v0, m = start(name)
    ora = DC.OracleFrames(CASE, [base()], recell=[np.eye(3)] if rule == "wrapped" else None)
    x, v, e, f = MR.run(x0 + np.array([dx, 0.0, 0.0]), v0, m, ora.md(), FLIGHTS[name][1], 1.0)
    return DC._frozen(dict(x=x, v=v, e=np.asarray(e), f=f, x_hist=np.array([t[0] for t in ora.trace]), x0=x0, v0=v0, m=m,
                           room=DC.window_room(ora.trace, [base()], DC.r_cut(CASE))))


def images_of(x, cell):
    """floor of the fractional coordinates: the cell image every atom lies in"""
    return np.floor(np.asarray(x) @ np.linalg.inv(cell)).astype(int)


@functools.lru_cache(maxsize=None)
def stored_wrapped(name, rewrap_every=7):
    """The storage of a wrapping object, restated: wrapped positions plus integer image counts, re-wrapped (x -= n . cell,
    img += n: a rounding) only in front of every ``rewrap_every``-th evaluation, the first included.  The forces are the
    crystal's at the stored positions, which is what the device's lists give between two builds (every neighbour within
    r_cut + skin of the build is on them, wherever the atom has gone since): the oracle behind its own fold.  On the stored
    positions as they are the oracle would not do: this projectile is 2.4 A outside the cell after six steps, the window has
    0.41 A of room, and the run then ends 4.6e-5 A away.  Unwrapped x, v, e, f at the end and the image counts."""
    x, v, m = start(name)
    a = base()
    cell = np.asarray(a.get_cell(), float)
    ora = DC.OracleFrames(CASE, [a], recell=[np.eye(3)])
    img = np.zeros((len(a), 3), dtype=int)
    ka = (ACC / m)[:, None]

    def evaluate(k, x, img):
        if k % rewrap_every == 0:
            n = images_of(x, cell)
            x, img = x - n @ cell, img + n
        return x, img, ora.md()(x)
    x, img, (e, f) = evaluate(0, x, img)
    for k in range(1, FLIGHTS[name][1] + 1):
        v = v + 0.5 * f * ka
        x = x + v
        x, img, (e, f) = evaluate(k, x, img)
        v = v + 0.5 * f * ka
    return DC._frozen(dict(x=x + img @ cell, v=v, e=np.asarray(e), f=f, img=img))
