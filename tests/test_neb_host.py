"""Host side of ``uf3_amd.forcefield.neb`` (no GPU): the NumPy restatement of the band optimiser (tests/_neb_ref.py) on the
Mueller-Brown surface -- one "atom" whose x, y are the surface's and whose z is harmonic -- finds the saddle with a climbing
image, leaves every image's force perpendicular to its tangent below fmax without one, keeps fixed atoms, freezes a band with a
NaN energy alone; ``interpolate`` with and without the minimum image on a skewed cell; and argument checks that raise before any
device call."""
import types

import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import neb
import _neb_ref as N
from _relax_ref import CONVERGED, NONFINITE

# Mueller & Brown (1979), the standard four terms
MB_A = np.array([-200.0, -100.0, -170.0, 15.0])
MB_a = np.array([-1.0, -1.0, -6.5, 0.7])
MB_b = np.array([0.0, 0.0, 11.0, 0.6])
MB_c = np.array([-10.0, -10.0, -6.5, 0.7])
MB_x0 = np.array([1.0, 0.0, -0.5, -1.0])
MB_y0 = np.array([0.0, 0.5, 1.5, 1.0])
KZ = 50.0
MIN_A, MIN_B = np.array([-0.5582236, 1.4417258]), np.array([-0.0500108, 0.4666941])
SADDLE, E_SADDLE = np.array([-0.822, 0.624]), -40.66
KW = dict(dt=0.002, dt_max=0.02, maxstep=0.05)          # the surface is stiff (curvatures of 1e2 .. 1e3): small steps


def muller_brown(p):
    """Energy and force [3] at p = (x, y, z)."""
    dx, dy = p[0] - MB_x0, p[1] - MB_y0
    t = MB_A * np.exp(MB_a * dx * dx + MB_b * dx * dy + MB_c * dy * dy)
    fx = -(t * (2 * MB_a * dx + MB_b * dy)).sum()
    fy = -(t * (MB_b * dx + 2 * MB_c * dy)).sum()
    return t.sum() + 0.5 * KZ * p[2] ** 2, np.array([fx, fy, -KZ * p[2]])


def evaluate(x):
    """Every row its own frame of one atom."""
    out = [muller_brown(p) for p in x]
    return np.array([o[0] for o in out]), np.array([o[1] for o in out])


def _line(m, z=0.3):
    """m images from minimum A to minimum B, the interior lifted off the plane so that z has something to relax."""
    x = np.zeros((m, 3))
    for k in range(m):
        x[k, :2] = MIN_A + (MIN_B - MIN_A) * k / (m - 1)
    x[1:-1, 2] = z
    return x


def test_forces_are_the_energys_gradient():
    p, h = np.array([-0.7, 0.9, 0.2]), 1e-6
    fd = np.array([-(muller_brown(p + h * np.eye(3)[k])[0] - muller_brown(p - h * np.eye(3)[k])[0]) / (2 * h) for k in range(3)])
    assert np.abs(fd - muller_brown(p)[1]).max() <= 1e-6
    for q in (MIN_A, MIN_B):
        assert np.abs(muller_brown(np.append(q, 0.0))[1]).max() < 1e-3


def test_climbing_image_finds_the_saddle():
    m = 9
    band = N.Band(evaluate, _line(m), np.arange(m + 1), [0, m], spring=50.0)
    band.run(2000, fmax=0.5, **KW)
    band.run(4000, fmax=0.01, climb=True, **KW)
    assert band.status.tolist() == [CONVERGED], (band.status, band.crit)
    ci = band.climbing[0]
    assert 0 < ci < m - 1
    e = evaluate(band.x)[0]
    assert ci == np.argmax(e)
    assert abs(e[ci] - E_SADDLE) <= 1e-2, e[ci]
    assert np.abs(band.x[ci, :2] - SADDLE).max() <= 1e-2, band.x[ci]
    assert abs(band.x[ci, 2]) <= 1e-2
    assert band.max_dr <= KW["maxstep"] * (1 + 1e-12)
    # the end points did not move
    assert np.array_equal(band.x[[0, -1]], _line(m)[[0, -1]])


def test_without_climbing_the_true_force_is_perpendicular_free():
    m, fmax = 8, 0.02
    band = N.Band(evaluate, _line(m), np.arange(m + 1), [0, m], spring=50.0)
    band.run(6000, fmax=fmax, **KW)
    assert band.status.tolist() == [CONVERGED] and band.climbing.tolist() == [-1]
    e, F = evaluate(band.x)
    for i in range(1, m - 1):
        tau = N.tangent(band.x[i + 1] - band.x[i], band.x[i] - band.x[i - 1], e[i - 1], e[i], e[i + 1])
        tau /= np.linalg.norm(tau)
        perp = F[i] - np.vdot(F[i], tau) * tau
        assert np.linalg.norm(perp) < fmax, (i, perp)
    assert e[1:-1].max() < E_SADDLE + 1e-9 and e[1:-1].max() > E_SADDLE - 15.0       # below the saddle, on the way over it


def test_fixed_atoms_never_move_and_do_not_count():
    # two "atoms" per image, each on its own copy of the surface; the second is fixed where it feels a large force
    m = 7
    x = np.zeros((m, 2, 3))
    x[:, 0] = _line(m)
    x[:, 1] = _line(m) + [0.05, -0.04, 0.1]
    x0 = x.reshape(-1, 3).copy()
    fixed = np.tile([False, True], m)

    def evaluate2(xx):
        e, F = evaluate(xx)
        return e.reshape(m, 2).sum(1), F
    band = N.Band(evaluate2, x0, 2 * np.arange(m + 1), [0, m], spring=50.0, fixed=fixed)
    band.run(6000, fmax=0.02, **KW)
    assert band.status.tolist() == [CONVERGED]
    assert np.array_equal(band.x[fixed], x0[fixed])
    assert not np.allclose(band.x[2:-2][~fixed[2:-2]], x0[2:-2][~fixed[2:-2]])
    F = evaluate2(band.x)[1]
    assert np.sqrt((F[fixed] ** 2).sum(1)).max() > 1.0               # forces the criterion did not see
    assert np.all(band.g[fixed] == 0.0) and np.all(band.v[fixed] == 0.0)


def test_a_nan_energy_freezes_only_its_band():
    m = 6
    x0 = np.concatenate([_line(m), _line(m)])
    calls = [0]

    def poisoned(x):
        e, F = evaluate(x)
        calls[0] += 1
        if calls[0] > 3:
            e[m + 2] = np.nan
        return e, F
    band = N.Band(poisoned, x0, np.arange(2 * m + 1), [0, m, 2 * m], spring=50.0)
    band.run(6000, fmax=0.02, **KW)
    assert band.status.tolist() == [CONVERGED, NONFINITE]
    assert band.steps[1] == 3 and band.steps[0] > 3
    alone = N.Band(evaluate, _line(m), np.arange(m + 1), [0, m], spring=50.0)
    alone.run(6000, fmax=0.02, **KW)
    assert alone.steps[0] == band.steps[0] and np.array_equal(alone.x, band.x[:m])      # and the other band did not notice


def test_split_runs_follow_one_run():
    m = 7
    one = N.Band(evaluate, _line(m), np.arange(m + 1), [0, m], spring=50.0)
    one.run(100, fmax=1e-6, climb=True, **KW)
    two = N.Band(evaluate, _line(m), np.arange(m + 1), [0, m], spring=50.0)
    two.run(40, fmax=1e-6, climb=True, **KW)
    two.run(60, fmax=1e-6, climb=True, **KW)
    assert np.array_equal(one.x, two.x) and one.steps.tolist() == two.steps.tolist() == [100]
    assert len(one.margins) == len(two.margins) == 101 and min(one.margins) > 0.0


def _skewed():
    cell = np.array([[4.0, 0.0, 0.0], [1.2, 3.8, 0.0], [0.4, 0.7, 5.0]])
    frac_a = np.array([[0.05, 0.95, 0.5], [0.5, 0.5, 0.1]])
    frac_b = np.array([[0.95, 0.05, 0.5], [0.55, 0.5, 0.9]])            # atom 0 crosses two faces, atom 1 one
    a = Atoms(numbers=[74, 42], positions=frac_a @ cell, cell=cell, pbc=True)
    b = Atoms(numbers=[74, 42], positions=frac_b @ cell, cell=cell, pbc=True)
    return cell, a, b


def test_interpolate_with_and_without_the_minimum_image():
    cell, a, b = _skewed()
    xa, xb = a.get_positions(), b.get_positions()
    plain = neb.interpolate(a, b, 5, mic=False)
    assert len(plain) == 5
    for k, im in enumerate(plain):
        assert np.allclose(im.get_positions(), xa + (xb - xa) * k / 4, atol=1e-14)
        assert np.array_equal(im.get_atomic_numbers(), [74, 42]) and np.array_equal(np.asarray(im.get_cell()), cell)
    wrapped = neb.interpolate(a, b, 5, mic=True)
    d = np.array([[-0.1, 0.1, 0.0], [0.05, 0.0, -0.2]]) @ cell            # the short way round
    for k, im in enumerate(wrapped):
        assert np.allclose(im.get_positions(), xa + d * k / 4, atol=1e-12)
    # the last image is final's periodic image, unwrapped: equal neighbour differences as stored
    steps = np.diff([im.get_positions() for im in wrapped], axis=0)
    assert np.allclose(steps, steps[0], atol=1e-12)
    shift = (wrapped[-1].get_positions() - xb) @ np.linalg.inv(cell)
    assert np.allclose(shift, np.round(shift), atol=1e-12) and np.abs(shift).max() > 0.5
    # a non-periodic axis is never wrapped
    slab_a = Atoms(numbers=[74, 42], positions=xa, cell=cell, pbc=[True, True, False])
    slab_b = Atoms(numbers=[74, 42], positions=xb, cell=cell, pbc=[True, True, False])
    last = neb.interpolate(slab_a, slab_b, 3)[-1].get_positions()
    assert np.allclose((last - xa) @ np.linalg.inv(cell), [[-0.1, 0.1, 0.0], [0.05, 0.0, 0.8]], atol=1e-12)
    free_a = Atoms(numbers=[74, 42], positions=xa, cell=np.zeros((3, 3)), pbc=False)
    free_b = Atoms(numbers=[74, 42], positions=xb, cell=np.zeros((3, 3)), pbc=False)
    assert np.allclose(neb.interpolate(free_a, free_b, 3)[1].get_positions(), (xa + xb) / 2)


@pytest.mark.parametrize("change,match", [
    (lambda b: Atoms(numbers=[74], positions=b.get_positions()[:1], cell=b.get_cell(), pbc=True), "atoms"),
    (lambda b: Atoms(numbers=[74, 74], positions=b.get_positions(), cell=b.get_cell(), pbc=True), "species"),
    (lambda b: Atoms(numbers=[74, 42], positions=b.get_positions(), cell=1.01 * np.asarray(b.get_cell()), pbc=True), "cell"),
    (lambda b: Atoms(numbers=[74, 42], positions=b.get_positions(), cell=b.get_cell(), pbc=[True, True, False]), "pbc")])
def test_interpolate_refuses_end_points_that_do_not_match(change, match):
    _, a, b = _skewed()
    with pytest.raises(ValueError, match=match):
        neb.interpolate(a, change(b), 5)
    with pytest.raises(ValueError, match="n_images"):
        neb.interpolate(a, b, 1)


class _NoDevice(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise _NoDevice()
    monkeypatch.setattr(_lib, "get_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def _band(m=4):
    _, a, b = _skewed()
    return neb.interpolate(a, b, m)


def _with(band, j, **kw):
    a = band[j]
    args = dict(numbers=a.get_atomic_numbers(), positions=a.get_positions(), cell=a.get_cell(), pbc=a.get_pbc())
    args.update(kw)
    out = list(band)
    out[j] = Atoms(**args)
    return out


@pytest.mark.parametrize("kw,match", [
    (dict(skin=-0.1), "skin"), (dict(skin=5.0), "skin"), (dict(bands=[]), "at least 3"), (dict(bands=_band(2)), "at least 3"),
    (dict(bands=[_band(4), _band(2)]), "band 1 has 2 images"), (dict(bands=_band()[0]), "list"),
    (dict(bands=_with(_band(), 2, numbers=[74, 74])), "species"),
    (dict(bands=_with(_band(), 1, cell=np.eye(3) * 6)), "cell"),
    (dict(bands=_with(_band(), 3, pbc=False)), "pbc"),
    (dict(bands=_band()[:2] + [Atoms(numbers=[74], positions=[[0, 0, 0]], cell=_band()[0].get_cell(), pbc=True)]), "atom count"),
    (dict(bands=_with(_band(), 2, positions=_band()[1].get_positions())), "identical"),
    (dict(bands=_with(_band(), 1, positions=[[np.nan, 0, 0], [1, 1, 1]])), "finite"),
    (dict(spring=0.0), "spring"), (dict(spring=float("inf")), "spring"), (dict(spring=[0.1, 0.2]), "spring"),
    (dict(fixed=[True, False]), "fixed holds 2"), (dict(fixed=[1, 0] * 4), "boolean"),
    (dict(fixed=[True, False] * 3 + [False, False]), "fixed mask differs")])
def test_constructor_checks_arguments_before_any_device_call(no_device, kw, match):
    args = dict(calc=types.SimpleNamespace(device=None), bands=_band())
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        neb.NudgedElasticBand(**args)


def test_valid_arguments_reach_the_device(no_device):
    calc = types.SimpleNamespace(device=None, bspline_config=None)
    with pytest.raises(_NoDevice):
        neb.NudgedElasticBand(calc, [_band(), _band(3)], spring=[0.1, 0.3], fixed=[True, False] * 7)


@pytest.mark.parametrize("kw,match", [
    (dict(max_steps=-1), "max_steps"), (dict(max_steps=2.5), "max_steps"), (dict(max_steps=True), "max_steps"),
    (dict(fmax=0.0), "fmax"), (dict(fmax=float("inf")), "fmax"), (dict(climb=1), "climb"), (dict(dt=-0.1), "dt"),
    (dict(dt_max=0.0), "dt_max"), (dict(maxstep=0.0), "maxstep"), (dict(check_every=0), "check_every"),
    (dict(record_every=-1), "record_every")])
def test_run_checks_arguments_before_any_device_call(no_device, kw, match):
    obj = neb.NudgedElasticBand.__new__(neb.NudgedElasticBand)
    obj.handle, obj.skin = None, 0.5
    args = dict(max_steps=10)
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        obj.run(**args)
    with pytest.raises(RuntimeError, match="closed"):
        obj.run(10)
