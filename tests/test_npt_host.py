"""Host side of constant-pressure dynamics (no GPU): the keyword checks of ``MolecularDynamics`` that raise before any device
call, the post-processing of its records, and the NumPy restatement of the integrator (tests/_npt_ref.py) on an analytic toy
potential with an exact virial -- a smoothly truncated Lennard-Jones solid with the minimum image -- which pins the equations
independently of the device: the dt^2 scaling of the NPH conserved quantity, time reversal, and the heavy-piston limit."""
import types

import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import md
import _md_ref
import _npt_ref


class _NoDevice(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise _NoDevice()
    monkeypatch.setattr(_lib, "get_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


def _pair(pbc=True):
    return Atoms(numbers=[74, 42, 74], positions=np.zeros((3, 3)), cell=np.eye(3) * 5, pbc=pbc)


def _args(**kw):
    args = dict(calculator=types.SimpleNamespace(device=None, bspline_config=None), atoms_or_list=_pair(), timestep_fs=1.0,
                masses={"W": 183.84, "Mo": 95.95}, temperature_K=300.0)
    args.update(kw)
    return args


@pytest.mark.parametrize("kw,match", [
    (dict(pressure_eV_A3=float("nan"), barostat_time_fs=100.0), "pressure_eV_A3"),
    (dict(pressure_eV_A3="high", barostat_time_fs=100.0), "pressure_eV_A3"),
    (dict(pressure_eV_A3=0.0), "barostat_time_fs"),
    (dict(pressure_eV_A3=0.0, barostat_time_fs=0.0), "barostat_time_fs"),
    (dict(pressure_eV_A3=0.0, barostat_time_fs=-5.0), "barostat_time_fs"),
    (dict(pressure_eV_A3=0.0, barostat_time_fs=100.0, barostat_friction_per_fs=-0.1), "barostat_friction_per_fs"),
    (dict(pressure_eV_A3=0.0, barostat_time_fs=100.0, piston_temperature_K=0.0), "piston_temperature_K"),
    (dict(pressure_eV_A3=0.0, barostat_time_fs=100.0, temperature_K=0.0), "piston_temperature_K"),
    (dict(barostat_time_fs=100.0), "need a pressure_eV_A3"),
    (dict(barostat_friction_per_fs=0.01), "need a pressure_eV_A3"),
    (dict(piston_temperature_K=300.0), "need a pressure_eV_A3"),
    (dict(pressure_eV_A3=0.0, barostat_time_fs=100.0, atoms_or_list=_pair(pbc=False)), "not periodic"),
    (dict(pressure_eV_A3=0.0, barostat_time_fs=100.0, atoms_or_list=[_pair(), _pair(pbc=[True, True, False])]), "frame 1 is not periodic")])
def test_constructor_checks_the_barostat_before_any_device_call(no_device, kw, match):
    with pytest.raises(ValueError, match=match):
        md.MolecularDynamics(**_args(**kw))


def test_valid_barostat_arguments_reach_the_device(no_device):
    for kw in (dict(pressure_eV_A3=-0.01, barostat_time_fs=200.0),
               dict(pressure_eV_A3=0.0, barostat_time_fs=200.0, temperature_K=0.0, piston_temperature_K=300.0, barostat_friction_per_fs=0.01)):
        with pytest.raises(_NoDevice):
            md.MolecularDynamics(**_args(**kw))


def test_run_checks_the_barostat_before_any_device_call(no_device):
    obj = md.MolecularDynamics.__new__(md.MolecularDynamics)
    obj.handle, obj.timestep_fs, obj.temperature_K, obj.friction_per_fs, obj.seed, obj.skin = None, 1.0, 300.0, 0.0, 0, 0.5
    obj.pressure_eV_A3, obj.barostat_time_fs, obj.barostat_friction_per_fs, obj.piston_temperature_K = 0.0, 100.0, 0.0, None
    obj.barostat_time_fs = -1.0
    with pytest.raises(ValueError, match="barostat_time_fs"):
        obj.run(10)
    obj.barostat_time_fs, obj.temperature_K = 100.0, 0.0
    with pytest.raises(ValueError, match="piston_temperature_K"):
        obj.run(10)
    obj.piston_temperature_K = 300.0
    with pytest.raises(RuntimeError, match="closed"):
        obj.run(10)


def test_npt_records_use_each_steps_volume():
    rng = np.random.default_rng(5)
    raw = rng.normal(size=(3, 2, 17))
    raw[..., 14] = rng.uniform(50, 60, (3, 2))
    out = md.npt_records(raw, [4, 5], 10, 5)
    assert out["step"].tolist() == [15, 20, 25]
    assert np.allclose(out["stress"], (raw[..., 2:8] - raw[..., 8:14]) / raw[..., 14:15], rtol=1e-14)
    assert np.allclose(out["pressure"], -out["stress"][..., :3].sum(-1) / 3, rtol=1e-14)
    assert np.array_equal(out["volume"], raw[..., 14]) and np.array_equal(out["cell_scale"], raw[..., 15])
    assert np.array_equal(out["conserved"], raw[..., 16])
    # 3 V P = tr K - tr W
    assert np.allclose(3 * out["volume"] * out["pressure"], raw[..., 8:11].sum(-1) - raw[..., 2:5].sum(-1), rtol=1e-12)


# ---- the restatement on an analytic potential -----------------------------------------------------------------------------------
EPS, SIG, RC, A0, MASS = 0.0104, 3.4, 4.6, 5.27, 40.0


def _fcc(n=2):
    base = np.array([[0, 0, 0], [0.5, 0.5, 0], [0.5, 0, 0.5], [0, 0.5, 0.5]])
    grid = np.array([[i, j, k] for i in range(n) for j in range(n) for k in range(n)])
    return ((grid[:, None, :] + base[None]).reshape(-1, 3)) * A0, n * A0


def _lj(box0):
    """evaluate(x, s) of 4 eps [(sig/r)^12 - (sig/r)^6] (1 - (r/rc)^2)^2 in the cubic cell s * box0 (minimum image, rc < box / 2):
    energy, forces and tr W = sum over pairs of phi'(r) r, the exact strain derivative's trace."""
    def evaluate(x, s):
        box = box0 * float(s[0])
        assert RC < 0.5 * box
        d = x[None, :, :] - x[:, None, :]
        d -= box * np.round(d / box)
        r2 = np.sum(d * d, axis=2)
        np.fill_diagonal(r2, np.inf)
        r = np.sqrt(r2)
        inside = r < RC
        rr = np.where(inside, r, 1.0)
        u6 = (SIG / rr) ** 6
        lj, dlj = 4 * EPS * (u6 * u6 - u6), 4 * EPS * (-12 * u6 * u6 + 6 * u6) / rr
        q = 1 - (rr / RC) ** 2
        sw, dsw = q * q, -4 * q * rr / RC ** 2
        phi = np.where(inside, lj * sw, 0.0)
        dphi = np.where(inside, dlj * sw + lj * dsw, 0.0)
        e = 0.5 * phi.sum()
        f = np.sum((dphi / rr)[:, :, None] * d, axis=1)
        return np.array([e]), f, np.array([0.5 * np.sum(dphi * rr)])
    return evaluate


def _start(temperature=40.0, seed=3):
    x0, box0 = _fcc()
    m = np.full(len(x0), MASS)
    off = np.array([0, len(x0)])
    v0 = _md_ref.init_velocities(m, off, temperature, seed, 0, exact=True)
    x0 = x0 + np.random.default_rng(seed).normal(0, 0.05, x0.shape)
    return x0, v0, m, off, box0


def test_toy_virial_is_the_energys_strain_derivative():
    x0, _, _, _, box0 = _start()
    ev = _lj(box0)
    h = 1e-6
    ep, em = ev(x0 * (1 + h), np.array([1 + h]))[0][0], ev(x0 * (1 - h), np.array([1 - h]))[0][0]
    assert (ep - em) / (2 * h) == pytest.approx(ev(x0, np.array([1.0]))[2][0], rel=1e-6)


P0, TAU = 0.0005, 500.0


def test_nph_conserved_quantity_error_scales_with_dt_squared():
    x0, v0, m, off, box0 = _start()
    ev = _lj(box0)
    drift = {}
    for dt in (4.0, 2.0):
        P = _npt_ref.Pistons(off, [box0 ** 3], TAU, 40.0)
        out = _npt_ref.run(x0, v0, m, P, [1.0], [0.0], ev, int(round(400 / dt)), dt, P0, history=True)
        hist = out[-1][:, 0]
        drift[dt] = np.abs(hist - hist[0]).max()
        assert abs(out[2][0] - 1.0) > 1e-3                   # (the cell did move)
    ratio = drift[4.0] / drift[2.0]
    assert 3.0 <= ratio <= 5.0, (drift, ratio)
    assert drift[4.0] < 0.05 * 32 * 1.5 * md.KB * 40.0, drift


def test_reversing_velocities_and_strain_rate_retraces_the_trajectory():
    x0, v0, m, off, box0 = _start()
    ev = _lj(box0)
    P = _npt_ref.Pistons(off, [box0 ** 3], TAU, 40.0)
    x1, v1, s1, ve1, _, _ = _npt_ref.run(x0, v0, m, P, [1.0], [0.0], ev, 60, 2.0, P0)
    assert np.abs(x1 - x0).max() > 0.05 and abs(s1[0] - 1.0) > 1e-4
    x2, v2, s2, ve2, _, _ = _npt_ref.run(x1, -v1, m, P, s1, -ve1, ev, 60, 2.0, P0)
    assert np.abs(x2 - x0).max() <= 1e-9
    assert np.abs(v2 + v0).max() <= 1e-10
    assert abs(s2[0] - 1.0) <= 1e-12 and abs(ve2[0]) <= 1e-14


def test_a_very_heavy_piston_at_rest_is_velocity_verlet():
    x0, v0, m, off, box0 = _start()
    ev = _lj(box0)
    P = _npt_ref.Pistons(off, [box0 ** 3], 1e12, 40.0)
    x1, v1, s1, ve1, e1, f1 = _npt_ref.run(x0, v0, m, P, [1.0], [0.0], ev, 50, 2.0, P0)
    one = np.array([1.0])
    xr, vr, er, fr = _md_ref.run(x0, v0, m, lambda x: ev(x, one)[:2], 50, 2.0)
    assert abs(s1[0] - 1.0) <= 1e-15
    assert np.abs(x1 - xr).max() <= 1e-12 * np.abs(xr).max()
    assert np.abs(v1 - vr).max() <= 1e-12 * np.abs(vr).max()
    assert abs(e1[0] - er[0]) <= 1e-12 * abs(er[0])


def test_phi_and_psi_series_meet_the_closed_forms():
    for x in (-3e-4, -1e-4 * (1 - 1e-9), 1e-4 * (1 - 1e-9), 3e-4, 1e-9, 0.0):
        assert float(_npt_ref.phi(x)) == pytest.approx(1 - x / 2 + x * x / 6 - x ** 3 / 24 + x ** 4 / 120, rel=1e-15)
        assert float(_npt_ref.psi(x)) == pytest.approx(1 + x / 2 + x * x / 6 + x ** 3 / 24 + x ** 4 / 120, rel=1e-15)
