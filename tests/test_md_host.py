"""Host side of ``uf3_amd.forcefield.md`` (no GPU): the Philox4x32-10 restatement the device kernels are held to, mass
resolution, unit constants, the post-processing of thermo records, and argument checks that raise before any device call."""
import types

import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import md
from _md_ref import init_velocities, normals3, philox

KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_restatement_reproduces_the_known_answers():
    for ctr, key, want in KAT:
        assert tuple(int(w) for w in philox([ctr], [key])[0]) == want


def test_normals_are_standard_and_depend_on_every_counter_word():
    z = normals3(7, np.arange(20000), 3, 0)
    assert z.shape == (20000, 3) and np.all(np.isfinite(z))
    assert abs(z.mean()) < 0.02 and abs(z.std() - 1.0) < 0.02
    base = normals3(7, [5], 3, 0)
    for other in (normals3(8, [5], 3, 0), normals3(7, [6], 3, 0), normals3(7, [5], 4, 0), normals3(7, [5], 3 + (1 << 32), 0),
                  normals3(7, [5], 3, 2)):
        assert not np.allclose(base, other)


def _pair():
    return Atoms(numbers=[74, 42, 74], positions=np.zeros((3, 3)), cell=np.eye(3) * 5, pbc=True)


def test_masses_from_a_dict_by_symbol_or_number():
    m = md.resolve_masses([_pair(), _pair()], {"W": 183.84, 42: 95.95})
    assert m.tolist() == [183.84, 95.95, 183.84] * 2


def test_masses_per_atom_and_from_get_masses():
    assert md.resolve_masses(_pair(), [1.0, 2.0, 3.0]).tolist() == [1.0, 2.0, 3.0]
    a = _pair()
    a.get_masses = lambda: np.array([4.0, 5.0, 6.0])
    assert md.resolve_masses([a], None).tolist() == [4.0, 5.0, 6.0]
    with pytest.raises(ValueError, match="masses for 3 atoms"):
        md.resolve_masses(_pair(), [1.0, 2.0])
    with pytest.raises(ValueError, match="positive"):
        md.resolve_masses(_pair(), [1.0, 0.0, 3.0])


def test_missing_masses_name_the_species():
    with pytest.raises(ValueError, match="no mass for Mo"):
        md.resolve_masses(_pair(), {"W": 183.84})
    with pytest.raises(ValueError, match="Mo, W"):
        md.resolve_masses(_pair(), None)


def test_unit_constants():
    # 2 amu at 1 A/fs: 1/2 m v^2 = 103.642... eV; ASE's time unit is sqrt of that factor in fs
    assert md.kinetic_energy([[1.0, 0.0, 0.0]], [2.0]) == pytest.approx(103.64269652680505, rel=1e-15)
    assert md.ASE_TIME_FS == pytest.approx(np.sqrt(md.KE_UNIT), rel=1e-6)
    assert md.ACC * md.KE_UNIT == pytest.approx(1.0, rel=1e-12)
    ke = 1.5 * 10 * md.KB * 300.0
    assert md.temperature(ke, 10) == pytest.approx(300.0, rel=1e-14)


def test_thermo_records_stress_pressure_and_temperature():
    rng = np.random.default_rng(3)
    n_rec, n_frames = 3, 2
    raw = rng.normal(size=(n_rec, n_frames, 14))
    vol = np.array([100.0, 0.0])                    # the second frame has no volume (a cluster)
    out = md.thermo_records(raw, [4, 5], vol, 10, 5, stress=True)
    assert out["step"].tolist() == [15, 20, 25]
    assert np.array_equal(out["potential_energy"], raw[..., 0])
    assert np.allclose(out["temperature"], 2 * raw[..., 1] / (3 * np.array([4, 5]) * md.KB))
    assert np.allclose(out["stress"][:, 0], (raw[:, 0, 2:8] - raw[:, 0, 8:14]) / 100.0)
    assert np.all(np.isnan(out["stress"][:, 1]))
    assert np.allclose(out["pressure"][:, 0], -out["stress"][:, 0, :3].sum(-1) / 3)
    # at rest (K = 0) the stress is W / V: UFCalculator.get_stress's sign
    raw[..., 8:14] = 0.0
    assert np.allclose(md.thermo_records(raw, [4, 5], vol, 0, 1, stress=True)["stress"][:, 0], raw[:, 0, 2:8] / 100.0)
    plain = md.thermo_records(raw[..., :2], [4, 5], vol, 0, 1)
    assert "stress" not in plain and plain["kinetic_energy"].shape == (n_rec, n_frames)


def test_host_initialisation_removes_the_centre_of_mass_and_hits_the_temperature():
    m = np.array([183.84] * 7 + [95.95] * 5)
    off = np.array([0, 7, 12])
    v = init_velocities(m, off, 500.0, 11, 0, exact=True)
    for lo, hi in zip(off[:-1], off[1:]):
        p = (m[lo:hi, None] * v[lo:hi]).sum(0)
        assert np.abs(p).max() <= 1e-12 * (m[lo:hi, None] * np.abs(v[lo:hi])).sum()
        assert md.temperature(md.kinetic_energy(v[lo:hi], m[lo:hi]), hi - lo) == pytest.approx(500.0, rel=1e-12)


class _NoDevice(Exception):
    pass


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise _NoDevice()
    monkeypatch.setattr(_lib, "get_context", refuse)
    monkeypatch.setattr(_lib, "load", refuse)


@pytest.mark.parametrize("kw,match", [
    (dict(timestep_fs=0.0), "timestep_fs"), (dict(timestep_fs=float("nan")), "timestep_fs"), (dict(timestep_fs=-1), "timestep_fs"),
    (dict(temperature_K=-1.0), "temperature_K"), (dict(temperature_K=float("inf")), "temperature_K"),
    (dict(friction_per_fs=-0.1), "friction_per_fs"), (dict(seed=-1), "seed"), (dict(seed=1 << 64), "seed"), (dict(seed=1.5), "seed"),
    (dict(skin=-0.1), "skin"), (dict(skin=5.0), "skin"), (dict(masses={"W": 183.84}), "no mass for Mo"),
    (dict(masses=[1.0, -2.0, 3.0]), "positive"), (dict(atoms_or_list=[]), "no frames")])
def test_constructor_checks_arguments_before_any_device_call(no_device, kw, match):
    args = dict(calculator=types.SimpleNamespace(device=None), atoms_or_list=_pair(), timestep_fs=1.0,
                masses={"W": 183.84, "Mo": 95.95})
    args.update(kw)
    with pytest.raises(ValueError, match=match):
        md.MolecularDynamics(**args)


def test_valid_arguments_reach_the_device(no_device):
    with pytest.raises(_NoDevice):
        md.MolecularDynamics(types.SimpleNamespace(device=None, bspline_config=None), _pair(), 1.0, masses={"W": 183.84, "Mo": 95.95})


def test_run_and_state_checks_arguments_before_any_device_call(no_device):
    obj = md.MolecularDynamics.__new__(md.MolecularDynamics)
    obj.handle, obj.timestep_fs, obj.temperature_K, obj.friction_per_fs, obj.seed, obj.skin = None, 1.0, 0.0, 0.0, 0, 0.5
    for bad in (dict(n_steps=-1), dict(n_steps=2.5), dict(n_steps=10, thermo_every=-1)):
        with pytest.raises(ValueError):
            obj.run(**bad)
    obj.timestep_fs = 0.0
    with pytest.raises(ValueError, match="timestep_fs"):
        obj.run(10)
    with pytest.raises(ValueError, match="temperature_K"):
        obj.initialize_velocities(-5.0)
    with pytest.raises(ValueError, match="seed"):
        obj.initialize_velocities(300.0, seed=-1)
    obj.timestep_fs = 1.0
    with pytest.raises(RuntimeError, match="closed"):
        obj.run(10)
