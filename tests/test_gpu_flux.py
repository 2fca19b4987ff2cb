"""Site energies, site virials and the heat current on the device (uf3_site_terms, uf3_heat_flux, uf3_md_run_flux) against
the NumPy restatement (_flux_ref), against the evaluator's own sums, their structural identities, and the MD sampling.

Tolerance against the restatement: the one tests/test_gpu_harmonic.py applies against _harmonic_ref, 1e-10 of each quantity's
largest magnitude; for J_pot, a sum of cancelling terms, 1e-10 of the sum of the terms' absolute values."""
import functools
import os

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator
from uf3_amd.forcefield.md import MolecularDynamics
from uf3_amd.regression import least_squares as ls
import _flux_ref as FR
from _util import GOLDEN, tensor_to_voigt

pytestmark = pytest.mark.gpu

RTOL = 1e-10
MASS = {10: 20.18, 42: 95.95, 54: 131.29, 74: 183.84}


@functools.lru_cache(maxsize=None)
def _model(name):
    if name == "mow_seeded":       # two species with 3-body terms on every trio: mixed-species triplets, one trio per lane
        basis = synthetic.notebook_basis(["Mo", "W"])
        model = ls.WeightedLinearModel(basis)
        coeff = np.random.default_rng(31).normal(0, 0.05, basis.n_feats)
        coeff[basis.col_idx] = 0.0
        model.coefficients = coeff
        return model
    return ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, name))


def _calc(name):
    return calculator.UFCalculator(_model(name), md_skin=0.0)


def _w16():
    return synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=3)


def _w2():
    return synthetic.lattice_frame("bcc", (1, 1, 1), 3.165, [74], seed=4)          # every atom neighbours its own images


def _w1():
    return Atoms(numbers=[74], positions=[[0.3, 0.1, 0.2]], cell=np.diag([3.165, 3.2, 3.1]), pbc=True)


def _nexe():
    return synthetic.lattice_frame("fcc", (1, 1, 1), 4.6, [10, 54], seed=5)


def _mow16():
    return synthetic.lattice_frame("bcc", (2, 2, 2), 3.2, [42, 74], seed=5)


def _cluster13():
    big = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=7)
    pos = np.asarray(big.get_positions(), dtype=float)
    keep = np.sort(np.argsort(np.linalg.norm(pos - pos.mean(axis=0), axis=1))[:13])
    return Atoms(numbers=np.full(13, 74), positions=pos[keep], cell=np.zeros((3, 3)), pbc=False)


def _w65():
    big = synthetic.lattice_frame("bcc", (3, 3, 4), 3.165, [74], seed=9)            # 72 sites, 7 vacancies
    keep = np.sort(np.random.default_rng(9).permutation(72)[:65])
    return Atoms(numbers=np.full(65, 74), positions=np.asarray(big.get_positions())[keep], cell=big.get_cell(), pbc=True)


def _vel(atoms, seed):
    return np.random.default_rng(seed).normal(0, 0.01, (len(atoms.get_atomic_numbers()), 3))


def _masses(atoms):
    return np.array([MASS[int(q)] for q in atoms.get_atomic_numbers()])


FRAMES = {"w16": ("model_unary.json", _w16, 21), "w2": ("model_unary.json", _w2, 22), "nexe4": ("model_binary.json", _nexe, 23),
          "w16_2and3": ("model_2and3.json", _w16, 24), "cluster13": ("model_unary.json", _cluster13, 25),
          "w1": ("model_unary.json", _w1, 26), "w65": ("model_unary.json", _w65, 27), "mow16": ("mow_seeded", _mow16, 28)}


@functools.lru_cache(maxsize=None)
def _reference(label):
    """U, W, J_conv, J_pot, scale of J_pot of one frame: computed once, shared, never changed."""
    model, make, seed = FRAMES[label]
    m = _model(model)
    atoms = make()
    ob = O.OracleBasis(m.bspline_config)
    coeff = np.asarray(m.coefficients, dtype=float)
    U, W = FR.site_terms(ob, atoms, coeff)
    Jc, Jp, scale = FR.heat_flux(ob, atoms, _vel(atoms, seed), _masses(atoms), coeff, with_scale=True)
    for a in (U, W, Jc, Jp, scale):
        a.setflags(write=False)
    return U, W, Jc, Jp, scale


def _check(label, U, W, flux):
    rU, rW, rJc, rJp, scale = _reference(label)
    assert np.abs(U - rU).max() <= RTOL * np.abs(rU).max(), (label, "U", np.abs(U - rU).max())
    assert np.abs(W - rW).max() <= RTOL * np.abs(rW).max(), (label, "W", np.abs(W - rW).max())
    assert np.abs(flux[0] - rJc).max() <= RTOL * np.abs(rJc).max(), (label, "J_conv", flux[0], rJc)
    assert scale.min() > 0
    assert np.all(np.abs(flux[1] - rJp) <= RTOL * scale), (label, "J_pot", flux[1], rJp, scale)


def _device(label):
    model, make, seed = FRAMES[label]
    calc, atoms = _calc(model), make()
    U, W = calc.site_terms([atoms])
    flux, Uf = calc.heat_flux([atoms], _vel(atoms, seed), _masses(atoms), site_energies=True)
    assert np.array_equal(Uf, U[0])
    return U[0], W[0], flux[0]


@pytest.mark.parametrize("label", ["w16", "w2", "nexe4", "w16_2and3", "cluster13", "mow16"])
def test_device_against_restatement(label):
    if label in ("nexe4", "mow16"):
        m = _masses(FRAMES[label][1]())
        assert len(set(m.tolist())) == 2                       # unequal masses in the binary cases
    if label == "mow16":                                       # both species among the neighbours: triplets of every leg order
        assert len(set(_mow16().get_atomic_numbers().tolist())) == 2
    _check(label, *_device(label))


BATCH = ["w16", "w1", "cluster13", "w65"]


def _batch_device():
    calc = _calc("model_unary.json")
    frames = [FRAMES[k][1]() for k in BATCH]
    vel = np.concatenate([_vel(a, FRAMES[k][2]) for k, a in zip(BATCH, frames)])
    masses = np.concatenate([_masses(a) for a in frames])
    U, W = calc.site_terms(frames)
    flux = calc.heat_flux(frames, vel, masses)
    return calc, frames, U, W, flux


def test_batch_against_restatement_and_alone():
    calc, frames, U, W, flux = _batch_device()
    sizes = [len(u) for u in U]
    assert sizes == [16, 1, 13, 65] and all(s % 64 for s in np.cumsum(sizes))      # no frame boundary on a wave boundary
    # a centre with more than 64 (j, k) pairs: the lane stride loops
    m = _model("model_unary.json").bspline_config
    r3 = m.r_max_map[("W", "W", "W")][0]
    pos, cell = np.asarray(frames[3].get_positions()), np.asarray(frames[3].get_cell())
    shifts = np.array([[a, b, c] for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)]) @ cell
    d = np.linalg.norm(pos[None, :, None, :] + shifts[None, None] - pos[:, None, None, :], axis=-1)
    n3 = ((d > m.r_min_map[("W", "W", "W")][0]) & (d <= r3)).sum(axis=(1, 2))
    assert (n3 * (n3 - 1) // 2).max() > 64
    for k, label in enumerate(BATCH):
        _check(label, U[k], W[k], flux[k])
    # a frame alone and inside the batch: the same bits
    for k in (0, 2):
        label = BATCH[k]
        Ua, Wa = calc.site_terms([frames[k]])
        fa = calc.heat_flux([frames[k]], _vel(frames[k], FRAMES[label][2]), _masses(frames[k]))
        assert np.array_equal(Ua[0], U[k]) and np.array_equal(Wa[0], W[k]) and np.array_equal(fa[0], flux[k])
    # two identical calls: the same bits
    _, _, U2, W2, flux2 = _batch_device()
    assert all(np.array_equal(a, b) for a, b in zip(U, U2)) and all(np.array_equal(a, b) for a, b in zip(W, W2))
    assert np.array_equal(flux, flux2)


def test_against_the_evaluator():
    calc, atoms = _calc("model_unary.json"), _w16()
    U, W = calc.site_terms([atoms])
    U, W = U[0], W[0]
    shares = np.array([calc.evaluate_atom_range(atoms, i, i + 1, forces=False)[0] for i in range(16)])
    assert np.abs(U - shares).max() <= 1e-12 * np.abs(shares).max()
    e, _, _, v = calc.evaluate_frames([atoms], forces=False, virial=True)
    assert abs(U.sum() - e[0]) <= 1e-12 * np.abs(U).sum()
    Ws = W.sum(axis=0)
    assert np.abs(tensor_to_voigt(0.5 * (Ws + Ws.T)) - v[0]).max() <= 1e-12 * np.abs(W).sum()
    # the ASE surfaces: per-atom energies, and per-atom stresses whose mean is get_stress
    assert np.array_equal(calc.get_potential_energies(atoms), U)
    s = calc.get_stresses(atoms)
    assert s.shape == (16, 6)
    stress = calc._get_stress(atoms)
    assert np.abs(s.mean(axis=0) - stress).max() <= 1e-12 * np.abs(s).max()


def test_tiling():
    """2 x 1 x 1: exactly the U list twice, J doubled within rounding.  Exactly, once the tiling itself is exact: the frame's
    coordinates and cell edges are multiples of 2^-20 A, so that `pos + cell[0]` and every image vector of the doubled cell
    have the bits they have in the single cell.  What is then left to differ is the order of each centre's entries (other
    atom numbers, other image shifts), which the kernel does not follow: it walks them in an order of the image vectors."""
    calc, atoms = _calc("model_unary.json"), _w16()
    q = 2.0 ** -20
    pos, cell = np.round(np.asarray(atoms.get_positions(), dtype=float) / q) * q, np.round(np.asarray(atoms.get_cell(), dtype=float) / q) * q
    vel, masses = _vel(atoms, 21), _masses(atoms)
    single = Atoms(numbers=np.full(16, 74), positions=pos, cell=cell, pbc=True)
    tiled = Atoms(numbers=np.full(32, 74), positions=np.concatenate([pos, pos + cell[0]]), cell=cell * np.array([[2], [1], [1]]),
                  pbc=True)
    assert np.array_equal(tiled.get_positions()[16:] - cell[0], pos)
    U, W = calc.site_terms([single])
    Ut, Wt = calc.site_terms([tiled])
    assert np.array_equal(Ut[0], np.concatenate([U[0], U[0]]))
    assert np.array_equal(Wt[0], np.concatenate([W[0], W[0]]))
    flux = calc.heat_flux([single], vel, masses)[0]
    ft = calc.heat_flux([tiled], np.concatenate([vel, vel]), np.concatenate([masses, masses]))[0]
    scale = _reference("w16")[4]                               # (the unrounded frame's: the same to 1e-6)
    assert np.abs(ft[0] - 2 * flux[0]).max() <= 1e-12 * np.abs(flux[0]).max()
    assert np.all(np.abs(ft[1] - 2 * flux[1]) <= 1e-12 * scale)


def test_lattice_shift():
    calc, atoms = _calc("model_unary.json"), _w16()
    pos, cell = np.asarray(atoms.get_positions(), dtype=float), np.asarray(atoms.get_cell(), dtype=float)
    vel, masses = _vel(atoms, 21), _masses(atoms)
    U, W = calc.site_terms([atoms])
    flux = calc.heat_flux([atoms], vel, masses)[0]
    scale = _reference("w16")[4]
    # one atom moved by a lattice vector
    moved = pos.copy()
    moved[5] += cell[0] - 2 * cell[2]
    shifted = Atoms(numbers=atoms.get_atomic_numbers(), positions=moved, cell=cell, pbc=True)
    Us, Ws = calc.site_terms([shifted])
    fs = calc.heat_flux([shifted], vel, masses)[0]
    assert np.abs(Us[0] - U[0]).max() <= 1e-12 * np.abs(U[0]).max()
    assert np.abs(Ws[0] - W[0]).max() <= 1e-12 * np.abs(W[0]).max()
    assert np.abs(fs[0] - flux[0]).max() <= 1e-12 * np.abs(flux[0]).max()
    assert np.all(np.abs(fs[1] - flux[1]) <= 1e-12 * scale)


def _md(friction, **kw):
    calc = _calc("model_unary.json")
    frames = [_w16(), synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=13)]
    dyn = MolecularDynamics(calc, frames, 1.0, masses={"W": MASS[74]}, temperature_K=600.0, friction_per_fs=friction, seed=7, **kw)
    dyn.initialize_velocities(600.0, seed=3)
    return calc, dyn


@pytest.mark.parametrize("friction", [0.0, 0.02], ids=["nve", "langevin"])
def test_md_records(friction):
    calc, dyn = _md(friction)
    rec = dyn.run(6, flux_every=2)
    assert rec["heat_flux"].shape == (3, 2, 3) and list(rec["flux_step"]) == [2, 4, 6]
    assert np.array_equal(rec["heat_flux"], rec["heat_flux_convective"] + rec["heat_flux_potential"])
    _, twin = _md(friction)
    masses = np.full(32, MASS[74])
    for k in range(3):
        twin.run(2)
        flux = calc.heat_flux(twin.get_atoms(), twin.get_velocities(), masses)
        # the same lists and kernels on the same bits: each part equal, bit for bit
        for q, name in enumerate(("heat_flux_convective", "heat_flux_potential")):
            assert np.array_equal(rec[name][k], flux[:, q]), (k, name, rec[name][k], flux[:, q])
    assert np.array_equal(twin.get_positions(), dyn.get_positions()) and np.array_equal(twin.get_velocities(), dyn.get_velocities())
    # run(4); run(2) = run(6), bit for bit
    _, split = _md(friction)
    a, b = split.run(4, flux_every=2), split.run(2, flux_every=2)
    for name in ("heat_flux_convective", "heat_flux_potential"):
        assert np.array_equal(np.concatenate([a[name], b[name]]), rec[name])
    assert list(b["flux_step"]) == [6]
    # the thermo records do not notice the samples
    _, one = _md(friction)
    _, two = _md(friction)
    r1, r2 = one.run(6, thermo_every=2, stress=True, flux_every=3), two.run(6, thermo_every=2, stress=True)
    for name in ("potential_energy", "kinetic_energy", "stress"):
        assert np.array_equal(r1[name], r2[name])
    assert r1["heat_flux"].shape == (2, 2, 3) and "heat_flux" not in r2
    for d in (dyn, twin, split, one, two):
        d.close()


def test_refusals():
    calc, atoms = _calc("model_unary.json"), _w16()
    vel, masses = _vel(atoms, 21), _masses(atoms)
    bad = masses.copy()
    bad[3] = 0.0
    with pytest.raises(_lib.UF3Error, match="masses must be positive"):
        calc.heat_flux([atoms], vel, bad)
    with pytest.raises(_lib.UF3Error, match="velocities must be"):
        calc.heat_flux([atoms], vel[:-1], masses)
    _, dyn = _md(0.02, pressure_eV_A3=0.0, barostat_time_fs=500.0)
    with pytest.raises(_lib.UF3Error, match="constant volume"):
        dyn.run(4, flux_every=2)
    dyn.close()


@pytest.mark.parametrize("label", ["w2", "nexe4"])
def test_optional_outputs_do_not_move_the_others(label):
    """The host entries' staging blocks hold an optional output only when it is asked for: the site energies have the same bits
    with and without the virials, the virials alone are the virials, and the current is the same with and without the site
    energies."""
    import ctypes as C
    model, make, seed = FRAMES[label]
    calc, atoms = _calc(model), make()
    U, W = calc.site_terms([atoms])
    assert np.array_equal(calc.site_terms([atoms], virials=False)[0][0], U[0])
    ctx = _lib.get_context(calc.device)
    db = _lib.device_basis(calc.bspline_config, ctx)
    batch = _lib.FrameBatch([atoms])
    w_only = np.full((batch.n_atoms, 3, 3), -7.0)
    addr = _lib._addr
    ctx.check(ctx.lib.uf3_site_terms(db.handle, C.byref(batch.struct), addr(batch.pos), addr(batch.z), calc._pc[0], calc._pc[1],
                                     calc._pc[2], None, addr(w_only)))
    assert np.array_equal(w_only, W[0])
    vel, m = _vel(atoms, seed), _masses(atoms)
    flux, Uf = calc.heat_flux([atoms], vel, m, site_energies=True)
    assert np.array_equal(calc.heat_flux([atoms], vel, m), flux) and np.array_equal(Uf, U[0])
    assert np.abs(flux).max() > 0
