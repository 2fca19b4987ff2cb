"""Host side of ``uf3_amd.forcefield.relax`` (no GPU): the NumPy restatement of per-frame FIRE (tests/_relax_ref.py) on an
analytic pair potential -- convergence, the first step's dt, the trust radius, fixed atoms, the cell force against central
differences of E(q, D) -- and argument checks that raise before any device call."""
import types

import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import relax
import _relax_ref as R

SHIFTS = np.array(list(np.ndindex(5, 5, 5))) - 2          # images out to two cells: the potential is negligible beyond


def _phi(r):
    """Two Gaussians: repulsive core, attractive shell (eV, Angstrom); returns phi and dphi/dr."""
    a, b = 20.0 * np.exp(-(r / 1.2) ** 2), np.exp(-(r / 1.8) ** 2)
    return a - b, -2 * r / 1.2 ** 2 * a + 2 * r / 1.8 ** 2 * b


def pair_energy(x, cell, periodic):
    """Energy, forces [n, 3] and W = dE/d(strain) (Voigt) of one frame."""
    n = len(x)
    e, F, W = 0.0, np.zeros((n, 3)), np.zeros((3, 3))
    shifts = SHIFTS @ cell if periodic else np.zeros((1, 3))
    for i in range(n):
        d = x[None, :, :] + shifts[:, None, :] - x[i]                   # [images, n, 3]
        r = np.sqrt((d * d).sum(-1))
        mask = r > 1e-9
        p, dp = _phi(np.where(mask, r, 1.0))
        p, dp = np.where(mask, p, 0.0), np.where(mask, dp, 0.0)
        e += 0.5 * p.sum()
        g = (dp / np.where(mask, r, 1.0))[..., None] * d                 # dphi/dr * d / r
        F[i] += g.sum((0, 1))
        W += 0.5 * np.einsum("kja,kjb->ab", g, d)
    return e, F, np.array([W[0, 0], W[1, 1], W[2, 2], W[1, 2], W[0, 2], W[0, 1]])


def _frames():
    rng = np.random.default_rng(5)
    a = 2.6
    grid = np.array(list(np.ndindex(2, 2, 2)), dtype=float)
    per = (grid * a + rng.normal(0, 0.12, grid.shape))
    cell = np.diag([2 * a, 2 * a, 2 * a]) @ np.array([[1.0, 0.04, 0.0], [0.0, 1.0, 0.03], [0.02, 0.0, 1.0]])
    cl = np.array(list(np.ndindex(2, 2, 1)), dtype=float) * 2.4 + rng.normal(0, 0.1, (4, 3))
    return [(per, cell, [True] * 3), (cl, np.zeros((3, 3)), [False] * 3)]


def _evaluator(frames):
    off = np.cumsum([0] + [len(f[0]) for f in frames])

    def evaluate(x, cells):
        es, Fs, Ws = [], [], []
        for k, (_, _, pbc) in enumerate(frames):
            e, F, W = pair_energy(x[off[k]:off[k + 1]], cells[k], all(pbc))
            es.append(e); Fs.append(F); Ws.append(W)
        return np.array(es), np.concatenate(Fs), np.array(Ws)
    return evaluate, off


@pytest.mark.parametrize("relax_cell", [False, True])
def test_restatement_converges_keeps_the_first_dt_and_the_trust_radius(relax_cell):
    frames = _frames()
    evaluate, off = _evaluator(frames)
    x0 = np.concatenate([f[0] for f in frames])
    fire = R.Fire(evaluate, x0, [f[1] for f in frames], [f[2] for f in frames], off, relax_cell=relax_cell)
    energies = fire.run(3000, fmax=1e-4, dt=0.05, maxstep=0.1)
    assert np.all(fire.status == R.CONVERGED), fire.status
    assert np.all(fire.steps > 10)
    assert sorted(fire.first_dt) == [(0, 0.05), (1, 0.05)]      # the first step keeps dt
    assert 0 < fire.max_dr <= 0.1 * (1 + 1e-12)
    assert np.all(energies[-1] < energies[0])
    e, F, W = evaluate(fire.x, fire.cells)
    assert np.sqrt((F * F).sum(1)).max() < 1e-4
    if relax_cell:
        G = R.cell_force(np.linalg.inv(fire.cell0[0]) @ fire.cells[0], R.voigt_to_matrix(W[0]), 8)
        assert np.sqrt((G * G).sum(1)).max() < 1e-4
        assert not np.allclose(fire.cells[0], fire.cell0[0])
        assert np.array_equal(fire.cells[1], fire.cell0[1])             # the cluster keeps its (empty) cell
    else:
        assert np.array_equal(fire.cells, fire.cell0)


def test_fixed_atoms_do_not_move_and_do_not_count():
    frames = _frames()
    evaluate, off = _evaluator(frames)
    x0 = np.concatenate([f[0] for f in frames])
    fixed = np.zeros(len(x0), bool)
    fixed[[1, 9]] = True
    fire = R.Fire(evaluate, x0, [f[1] for f in frames], [f[2] for f in frames], off, fixed=fixed)
    fire.run(3000, fmax=1e-4)
    assert np.all(fire.status == R.CONVERGED)
    assert np.array_equal(fire.x[fixed], x0[fixed])
    F = evaluate(fire.x, fire.cells)[1]
    assert np.sqrt((F[~fixed] ** 2).sum(1)).max() < 1e-4
    with pytest.raises(ValueError):
        R.Fire(evaluate, x0, [f[1] for f in frames], [f[2] for f in frames], off, relax_cell=True, fixed=fixed)


def test_non_finite_forces_freeze_only_their_frame():
    frames = _frames()
    evaluate, off = _evaluator(frames)

    def poisoned(x, cells):
        e, F, W = evaluate(x, cells)
        F[off[1]] = np.nan
        return e, F, W
    x0 = np.concatenate([f[0] for f in frames])
    fire = R.Fire(poisoned, x0, [f[1] for f in frames], [f[2] for f in frames], off)
    fire.run(3000, fmax=1e-4)
    assert fire.status.tolist() == [R.CONVERGED, R.NONFINITE]
    assert fire.steps[1] == 0 and np.array_equal(fire.x[off[1]:], x0[off[1]:])


def test_cell_force_matches_central_differences_of_the_energy():
    per, cell0, _ = _frames()[0]
    n = len(per)
    D = np.array([[1.01, 0.02, -0.01], [0.005, 0.99, 0.015], [-0.02, 0.01, 1.03]])
    q = per @ np.linalg.inv(D) + 0.03                # x = q D

    def energy(D_):
        return pair_energy(q @ D_, cell0 @ D_, True)[0]
    _, _, W = pair_energy(q @ D, cell0 @ D, True)
    G = R.cell_force(D, R.voigt_to_matrix(W), n)
    h = 1e-5
    fd = np.zeros((3, 3))
    for i in range(3):
        for j in range(3):
            dp, dm = D.copy(), D.copy()
            dp[i, j] += h
            dm[i, j] -= h
            fd[i, j] = -(energy(dp) - energy(dm)) / (2 * h) / n      # -dE/dY, Y = n D
    assert np.abs(G - fd).max() <= 1e-7, np.abs(G - fd).max()
    # and the force on q is F D^T: -dE/dq by central differences
    _, F, _ = pair_energy(q @ D, cell0 @ D, True)
    k = 3
    fdq = np.zeros(3)
    for a in range(3):
        qp, qm = q.copy(), q.copy()
        qp[k, a] += h
        qm[k, a] -= h
        fdq[a] = -(pair_energy(qp @ D, cell0 @ D, True)[0] - pair_energy(qm @ D, cell0 @ D, True)[0]) / (2 * h)
    assert np.abs((F @ D.T)[k] - fdq).max() <= 1e-7


class _NoDevice(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise _NoDevice()
    monkeypatch.setattr(_lib, "get_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def _pair():
    return Atoms(numbers=[74, 42, 74], positions=np.eye(3), cell=np.eye(3) * 5, pbc=True)


@pytest.mark.parametrize("kw,match", [
    (dict(skin=-0.1), "skin"), (dict(skin=5.0), "skin"), (dict(skin=float("nan")), "skin"), (dict(relax_cell=1), "relax_cell"),
    (dict(atoms_or_list=[]), "no frames"), (dict(fixed=[True, False]), "fixed holds 2"), (dict(fixed=[1, 0, 0]), "boolean"),
    (dict(fixed=[True, False, False], relax_cell=True), "relax_cell"),
    (dict(atoms_or_list=Atoms(numbers=[74], positions=[[np.nan, 0, 0]], cell=np.eye(3), pbc=True)), "finite")])
def test_constructor_checks_arguments_before_any_device_call(no_device, kw, match):
    args = dict(calc=types.SimpleNamespace(device=None), atoms_or_list=_pair())
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        relax.Relaxation(**args)


def test_valid_arguments_reach_the_device(no_device):
    with pytest.raises(_NoDevice):
        relax.Relaxation(types.SimpleNamespace(device=None, bspline_config=None), [_pair()], fixed=[True, False, False])


@pytest.mark.parametrize("kw,match", [
    (dict(max_steps=-1), "max_steps"), (dict(max_steps=2.5), "max_steps"), (dict(max_steps=True), "max_steps"),
    (dict(fmax=0.0), "fmax"), (dict(fmax=float("inf")), "fmax"), (dict(dt=-0.1), "dt"), (dict(dt_max=0.0), "dt_max"),
    (dict(maxstep=0.0), "maxstep"), (dict(check_every=0), "check_every"), (dict(record_every=-1), "record_every")])
def test_run_checks_arguments_before_any_device_call(no_device, kw, match):
    obj = relax.Relaxation.__new__(relax.Relaxation)
    obj.handle, obj.skin = None, 0.5
    args = dict(max_steps=10)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        obj.run(**args)
    with pytest.raises(RuntimeError, match="closed"):
        obj.run(10)
