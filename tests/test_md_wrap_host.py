"""Periodic wrapping and the mean-squared displacement of ``MolecularDynamics``: what can be held without a device.

(a) the references of tests/test_gpu_md_wrap.py bite: in the projectile runs of tests/_msd_ref.py an atom of the 16-atom Mo/W
    cell crosses cell faces, the oracle's energy of the unwrapped positions is no longer the crystal's, and a run that stores
    wrapped positions plus image counts and folds them only now and then reproduces the every-step one to rounding;
(b) the NumPy restatement of the MSD record and ``md.msd_records`` against direct formulas; ``md.diffusion_coefficient``;
(c) argument checks of the Python layer that never touch the device."""
import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.forcefield import md
import _driver_cells as DC
import _msd_ref as MS


# ------------------------------------------------------------------------------------------------------------ (a) the references
def test_the_projectile_leaves_the_window_and_the_unwrapped_rule_loses_its_interactions():
    """40 NVE steps, atom 3 at 0.4 A/fs more: it ends in cell image (2, 0, 1), 9.6 A outside the window of DESIGN.md section 7, and
    the reference that evaluates the unwrapped positions differs from the one that folds them into the cell in front of every
    evaluation by more than 0.1 eV.  (If a fixture change ever makes this fail the input tests nothing: lengthen the flight.)"""
    un, wr = MS.flight("fast", "unwrapped"), MS.flight("fast", "wrapped")
    cell = np.asarray(MS.base().get_cell(), float)
    de, dx = abs(un["e"][0] - wr["e"][0]), np.abs(un["x"] - wr["x"]).max()
    print(f"unwrapped against wrapped evaluation: {de:.3e} eV, {dx:.3e} A; window room {un['room']:.2f} A, atom {MS.ATOM} in "
          f"image {MS.images_of(wr['x'], cell)[MS.ATOM]}")
    assert de > 0.1
    assert un["room"] < 0 and wr["room"] < 0
    assert tuple(MS.images_of(wr["x"], cell)[MS.ATOM]) == (2, 0, 1)


def test_the_slow_projectile_bites_too():
    """30 steps at 0.2 A/fs (the early-warning path of the device test): room -0.35 A, 9.7e-3 eV."""
    un, wr = MS.flight("slow", "unwrapped"), MS.flight("slow", "wrapped")
    de = abs(un["e"][0] - wr["e"][0])
    print(f"slow flight: unwrapped against wrapped evaluation {de:.3e} eV, window room {un['room']:.2f} A")
    assert un["room"] < 0 and de > 1e-3


def test_the_wrapped_reference_is_well_conditioned():
    """Start positions moved by 1e-13 A move the end by about as much: the 1e-9 of the device test is a bound on arithmetic."""
    a, b = MS.flight("fast", "wrapped"), MS.flight("fast", "wrapped", 1e-13)
    d = np.abs(b["x"] - a["x"]).max()
    print(f"1e-13 A at the start: {d:.2e} A at the end")
    assert d < 1e-11


@pytest.mark.parametrize("name", sorted(MS.FLIGHTS))
def test_stored_wrapped_positions_with_image_counts_reproduce_the_every_step_reference(name):
    """Wrapped positions plus integer image counts, re-wrapped only in front of every 7th evaluation (forces of the crystal at
    the stored positions): within 1e-12 of the reference that folds in front of every evaluation.  The roundings of a wrap and
    of pos + img . cell stay far inside the device test's 1e-9, so wrapping in front of list builds only is enough."""
    ref, got = MS.flight(name, "wrapped"), MS.stored_wrapped(name)
    fig = dict(x=np.abs(got["x"] - ref["x"]).max(), v=np.abs(got["v"] - ref["v"]).max(), e=abs(got["e"][0] - ref["e"][0]),
               f=np.abs(got["f"] - ref["f"]).max())
    print(f"{name}: stored-wrapped, re-wrapped every 7th step, against the every-step reference: {fig}")
    assert max(fig.values()) < 1e-12
    if name == "fast":
        assert tuple(got["img"][MS.ATOM]) == (2, 0, 1)


# ---------------------------------------------------------------------------------------------------------- (b) the MSD on the host
def _two_frames():
    rng = np.random.default_rng(3)
    off = np.array([0, 7, 12])
    species = np.array([0, 1, 1, 0, 2, 0, 1, 1, 1, 1, 0, 1])          # (the second frame lacks species 2)
    masses = np.array([96.0, 180.0, 50.0])[species] * rng.uniform(0.9, 1.1, 12)
    origin = rng.normal(0, 3.0, (12, 3))
    x = origin + rng.normal(0, 2.0, (12, 3)) + np.array([0.7, -0.2, 0.4])
    return x, origin, masses, species, off


def test_msd_records_equal_the_direct_formulas():
    x, origin, masses, species, off = _two_frames()
    raw = np.array([MS.record(x, origin, masses, species, off, 3), MS.record(0.5 * (x + origin), origin, masses, species, off, 3)])
    assert raw.shape == (2, 2, 16)
    counts = np.array([[np.sum(species[lo:hi] == q) for q in range(3)] for lo, hi in zip(off[:-1], off[1:])])
    rec = md.msd_records(raw, counts, 100, 5)
    assert np.array_equal(rec["msd_step"], [105, 110])
    for k, xk in enumerate((x, 0.5 * (x + origin))):
        msd, msd_all, com, com_all = MS.direct(xk, origin, masses, species, off, 3)
        for key, ref in (("msd", msd), ("msd_all", msd_all), ("msd_com_removed", com), ("msd_all_com_removed", com_all)):
            assert rec[key][k].shape == ref.shape
            assert np.array_equal(np.isnan(rec[key][k]), np.isnan(ref)), key
            assert np.allclose(rec[key][k], ref, rtol=1e-13, atol=1e-13, equal_nan=True), key
    assert np.isnan(rec["msd"][0, 1, 2]) and not np.isnan(rec["msd"][0, 0]).any()
    # (a rigid shift of every atom is a centre-of-mass displacement: it drops out of the com-removed figures alone)
    shifted = np.array([MS.record(x + 5.0, origin, masses, species, off, 3)])
    rs = md.msd_records(shifted, counts, 0, 1)
    assert np.allclose(rs["msd_all_com_removed"][0], rec["msd_all_com_removed"][0], rtol=1e-12)
    assert np.all(rs["msd_all"][0] > rec["msd_all"][0] + 10.0)
    with pytest.raises(ValueError, match="msd_records"):
        md.msd_records(raw[..., :12], counts, 0, 1)


def test_diffusion_coefficient_on_a_synthetic_line():
    dt, D = 2.5, 0.0123
    t = dt * np.arange(1, 41)
    line = 6.0 * D * t + 0.4
    assert md.diffusion_coefficient(line, dt) == pytest.approx(D, rel=1e-12)
    # ballistic start, linear tail: only the fit over the tail gives the slope
    bent = np.where(t < 30.0, 0.01 * t * t, 6.0 * D * t + 0.4)
    assert md.diffusion_coefficient(bent, dt, fit_from=0.5) == pytest.approx(D, rel=1e-12)
    assert abs(md.diffusion_coefficient(bent, dt, fit_from=0.0) - D) > 1e-4
    both = md.diffusion_coefficient(np.stack([line, 2.0 * line], axis=1), dt)
    assert both.shape == (2,) and np.allclose(both, [D, 2.0 * D], rtol=1e-12)
    for bad in (dict(msd=line[:1]), dict(sample_time_fs=0.0), dict(fit_from=1.5), dict(fit_from=-0.1)):
        kw = dict(msd=line, sample_time_fs=dt)
        kw.update(bad)
        with pytest.raises(ValueError, match="diffusion_coefficient"):
            md.diffusion_coefficient(**kw)


# ------------------------------------------------------------------------------------------- (c) checks that never touch the device
def _bare(**attrs):
    dyn = object.__new__(md.MolecularDynamics)
    for k, v in dict(timestep_fs=1.0, temperature_K=0.0, friction_per_fs=0.0, skin=0.5, seed=0, **attrs).items():
        setattr(dyn, k, v)
    return dyn


def test_python_argument_checks_never_touch_the_device():
    with pytest.raises(ValueError, match="MolecularDynamics: wrap must be True or False"):
        md.MolecularDynamics(None, [MS.base()], 1.0, masses=DC.MASSES, wrap="yes")
    with pytest.raises(ValueError, match="MolecularDynamics: wrap must be True or False"):
        md.MolecularDynamics(None, [MS.base()], 1.0, masses=DC.MASSES, wrap=1)
    dyn = _bare()
    assert dyn.wrap is False
    for bad in (-1, 2.0, True, None):
        with pytest.raises(ValueError, match="MolecularDynamics: msd_every"):
            dyn.run(10, msd_every=bad)
    with pytest.raises(_lib.UF3Error, match="uf3_md_run_msd: msd_every does not go into one run") as err:
        dyn.run(10, msd_every=2, flux_every=2)
    assert err.value.code == 1
    with pytest.raises(_lib.UF3Error, match="uf3_md_run_msd: msd_every does not go into one run"):
        dyn.run(10, msd_every=2, grade_every=5)
    baro = _bare(pressure_eV_A3=0.0, barostat_time_fs=500.0, barostat_friction_per_fs=0.0, piston_temperature_K=300.0)
    with pytest.raises(_lib.UF3Error, match="uf3_md_run_msd: .*constant volume only") as err:
        baro.run(10, msd_every=2)
    assert err.value.code == 1
