"""Periodic wrapping with image counts (``k_md_wrap``, ``MolecularDynamics(wrap=True)``) and the mean-squared displacement
(``k_md_msd_partial``, ``k_md_msd_frame``, ``run(msd_every=k)``) on the device.

The references are the oracle's alone (tests/_msd_ref.py; tests/test_md_wrap_host.py shows that they bite): a projectile that
crosses cell faces, against ``_md_ref.run`` driven by the oracle behind a fold into the cell.  Bounds: 1e-9 on positions,
velocities and energies (tests/test_gpu_md.py's TOL; the reference moves by 3e-13 for 1e-13 at the start), 1e-8 max|F| on
forces, 1e-10 for blocks against one run (the existing blocks test's), 1e-12 for quantities that only pass through a wrap."""
import ctypes as C
import functools

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator, md
import _driver_cells as DC
import _msd_ref as MS
import test_redescribed_host as RH
import test_site_redescribed_host as SH
from test_gpu_md import _cluster, _w128

pytestmark = pytest.mark.gpu
TOL = 1e-9
FTOL = 1e-8
BLOCK_TOL = 1e-10
ZS = [42, 74]                                   # the Mo/W basis' species, ascending


@functools.lru_cache(maxsize=None)
def _calc():
    return calculator.UFCalculator(DC.model("bcc_mow"), md_skin=0.0)


@functools.lru_cache(maxsize=None)
def _graded_calc():
    return calculator.UFCalculator(SH.posterior("bcc_mow"), md_skin=0.0)


def _ctx():
    return _lib.get_context(_calc().device)


def _dynamics(frames, vel=None, calc=None, **kw):
    kw.setdefault("masses", DC.MASSES)
    dyn = md.MolecularDynamics(calc or _calc(), frames, 1.0, **kw)
    if vel is not None:
        dyn.set_velocities(vel)
    return dyn


def _state(dyn):
    return dict(x=dyn.get_positions(), v=dyn.get_velocities(), e=dyn.get_potential_energies(), f=dyn.get_forces())


def _figures(got, ref):
    return dict(x=float(np.abs(got["x"] - ref["x"]).max()), v=float(np.abs(got["v"] - ref["v"]).max()),
                e=float((np.abs(got["e"] - ref["e"]) / np.maximum(1.0, np.abs(ref["e"]))).max()),
                f=float(np.abs(got["f"] - ref["f"]).max() / max(1.0, np.abs(ref["f"]).max())))


def _inside(x, cell, pbc=(True, True, True)):
    frac = np.asarray(x) @ np.linalg.inv(np.asarray(cell, float))
    per = np.asarray(pbc, bool)
    return bool(np.all(frac[:, per] >= -1e-12) and np.all(frac[:, per] < 1.0 + 1e-12))


# =============================================================================================== 1. crossing, against the oracle
@functools.lru_cache(maxsize=None)
def _flight(name, skin, wrap, blocks=None, msd_every=0):
    x0, v0, m = MS.start(name)
    n = MS.FLIGHTS[name][1]
    st0 = _ctx().md_stats()
    recs = []
    with _dynamics([MS.base()], v0, skin=skin, wrap=wrap) as dyn:
        for k in blocks or (n,):
            recs.append(dyn.run(k, thermo_every=1, msd_every=msd_every))
        assert dyn.step == n
        out = _state(dyn)
        out.update(img=dyn.get_images(), wrapped=dyn.get_positions(wrap=True), rec=recs[-1], recs=recs, atoms=dyn.get_atoms()[0])
    st1 = _ctx().md_stats()
    out["stats"] = {k: st1[k] - st0[k] for k in st0}
    return out


@pytest.mark.parametrize("name,skin", [("fast", 0.5), ("fast", 0.0), ("slow", 1.0)], ids=["outrun-skin0.5", "rebuild-skin0", "early-skin1.0"])
def test_a_projectile_that_crosses_cell_faces_follows_the_oracle_driven_restatement(name, skin):
    """The test that fails without the feature.  skin 0.5: a step of 0.4 A exceeds skin / 2, every step is the "lists outrun"
    repeat; skin 0: the rebuild-everything route; the slow flight at skin 1.0: the early-warning rebuild."""
    ref, got = MS.flight(name, "wrapped"), _flight(name, skin, True)
    cell = np.asarray(MS.base().get_cell(), float)
    fig = _figures(got, ref)
    print(f"{name} flight, skin {skin}, wrap=True against the oracle-driven restatement: {fig}; list statistics {got['stats']}")
    assert max(fig["x"], fig["v"], fig["e"]) <= TOL and fig["f"] <= FTOL, fig
    if skin == 0.5:
        assert got["stats"]["redone"] > 0
    if skin == 1.0:
        assert got["stats"]["builds"] > 1
    want = MS.images_of(ref["x"], cell)
    if name == "fast":
        assert tuple(got["img"][MS.ATOM]) == (2, 0, 1)
    # stored position + images @ cell is the position; the stored position is inside the cell up to the moves since the last wrap
    stored = got["x"] - got["img"] @ cell
    assert np.abs(got["img"] - want).max() <= 1 and np.abs(MS.images_of(stored, cell)).max() <= 1
    assert _inside(got["wrapped"], cell)
    assert np.abs(got["atoms"].get_positions() - got["x"]).max() == 0.0
    # the input bites: the same run without wrapping ends somewhere else
    plain = _flight(name, skin, False)
    away = float(np.abs(plain["e"] - ref["e"]).max())
    print(f"  wrap=False ends {away:.3e} eV away from the reference")
    assert away > (0.1 if name == "fast" else 1e-3)
    assert not plain["img"].any()


# ================================================================================================================ 2. descriptions
def _pair_runs(name, langevin, n_steps=30):
    inside, outside = RH.unwrapped_frames()[name]
    vel = RH.velocities("bcc_mow", DC.ORIGINAL)
    out = {}
    for key, atoms in (("inside", inside), ("outside", outside)):
        with _dynamics([atoms], vel, wrap=True, temperature_K=300.0 if langevin else 0.0, friction_per_fs=0.05 if langevin else 0.0,
                       seed=DC.MD_SEED) as dyn:
            img0 = dyn.get_images()
            e0, f0 = dyn.get_potential_energies(), dyn.get_forces()
            rec = dyn.run(n_steps, thermo_every=1)
            out[key] = dict(img0=img0, e0=e0, f0=f0, rec=rec, x=dyn.get_positions(), img=dyn.get_images())
    return inside, outside, out


@pytest.mark.parametrize("name", ["one_atom", "every_atom"])
def test_a_wrapping_object_describes_the_crystal_wherever_its_atoms_were_given(name):
    cell = np.asarray(RH.CASES["bcc_mow"][0].get_cell(), float)
    for langevin in (False, True):
        inside, outside, r = _pair_runs(name, langevin)
        moved = np.rint((outside.get_positions() - inside.get_positions()) @ np.linalg.inv(cell)).astype(int)
        assert np.abs(moved).max() >= 2
        a, b = r["inside"], r["outside"]
        # the images at the start are the integers the fixture moved by (the wrapped frame's own are zero)
        assert not a["img0"].any() and np.array_equal(b["img0"], moved)
        de = abs(b["e0"][0] - a["e0"][0]) / abs(a["e0"][0])
        df = np.abs(b["f0"] - a["f0"]).max() / np.abs(a["f0"]).max()
        dr = np.abs(b["rec"]["potential_energy"] - a["rec"]["potential_energy"]).max()
        dk = np.abs(b["rec"]["kinetic_energy"] - a["rec"]["kinetic_energy"]).max()
        dx = np.abs(b["x"] - a["x"] - moved @ cell).max()
        print(f"{name} langevin={langevin}: step 0 dE {de:.2e}, dF {df:.2e}; 30 steps: PE {dr:.2e}, KE {dk:.2e} eV; "
              f"unwrapped positions minus the given lattice vectors {dx:.2e} A")
        assert de <= 1e-12 and df <= 1e-12
        assert dr <= TOL and dk <= TOL and dx <= TOL


# ========================================================================================================================== 3. NPT
def test_a_wrapping_object_at_a_pressure_wraps_against_the_current_cell():
    inside, outside = RH.unwrapped_frames()["every_atom"]
    vel = RH.velocities("bcc_mow", DC.ORIGINAL)
    cell0 = np.asarray(inside.get_cell(), float)
    moved = np.rint((outside.get_positions() - inside.get_positions()) @ np.linalg.inv(cell0)).astype(int)
    r = {}
    for key, atoms in (("inside", inside), ("outside", outside)):
        with _dynamics([atoms], vel, wrap=True, temperature_K=300.0, seed=DC.MD_SEED, pressure_eV_A3=DC.NPT_KW["p0"],
                       barostat_time_fs=DC.NPT_KW["tau"]) as dyn:
            rec = dyn.run(20, thermo_every=1)
            r[key] = dict(rec=rec, x=dyn.get_positions(), cell=dyn.cells[0], img=dyn.get_images(), s=dyn.cell_scales,
                          wrapped=dyn.get_positions(wrap=True))
    a, b = r["inside"], r["outside"]
    fig = {k: float(np.abs(b["rec"][k] - a["rec"][k]).max()) for k in ("volume", "potential_energy", "cell_scale")}
    fig["volume"] /= float(a["rec"]["volume"].max())
    assert abs(a["s"][0] - 1.0) > 1e-4                          # (the cell has changed: the original cell would not do below)
    dx = np.abs(b["x"] - a["x"] - moved @ b["cell"]).max()
    dx_old = np.abs(b["x"] - a["x"] - moved @ cell0).max()
    print(f"NPH, 20 steps: {fig}, cell scale {a['s'][0]:.6f}; unwrapped positions minus n . cell(t) {dx:.2e} A (n . cell(0): {dx_old:.2e})")
    assert max(fig.values()) <= TOL and np.abs(b["cell"] - a["cell"]).max() <= TOL
    assert dx <= TOL and dx_old > 1e-4
    assert _inside(b["wrapped"], b["cell"])


# ================================================================================================= 4. samplers on a wrapping object
def test_flux_and_grade_samples_of_a_wrapping_object_do_not_depend_on_where_atoms_were_given():
    inside, outside = RH.unwrapped_frames()["every_atom"]
    vel = RH.velocities("bcc_mow", DC.ORIGINAL)
    r = {}
    for key, atoms in (("inside", inside), ("outside", outside)):
        with _dynamics([atoms], vel, wrap=True) as dyn:
            flux = dyn.run(20, flux_every=5)
        with _dynamics([atoms], vel, calc=_graded_calc(), wrap=True) as dyn:
            grade = dyn.run(20, grade_every=5)
        r[key] = dict(flux=flux, grade=grade)
    a, b = r["inside"], r["outside"]
    fig = {}
    for k in ("heat_flux_convective", "heat_flux_potential"):
        fig[k] = float(np.abs(b["flux"][k] - a["flux"][k]).max() / max(1.0, np.abs(a["flux"][k]).max()))
    fig["grade"] = float((np.abs(b["grade"]["grade"] - a["grade"]["grade"]) / np.maximum(1.0, a["grade"]["grade"])).max())
    print(f"flux and grade records, atoms given outside against inside: {fig}")
    assert a["flux"]["heat_flux"].shape == (4, 1, 3) and a["grade"]["grade"].shape == (4, 1)
    assert np.abs(a["flux"]["heat_flux_potential"]).max() > 1e-6
    assert max(fig.values()) <= TOL
    assert np.array_equal(a["grade"]["grade_atom"], b["grade"]["grade_atom"])


# ========================================================================================================================== 5. MSD
def _msd_reference(x_hist, origin, every, atoms_list, masses, magnitudes=False):
    off = np.cumsum([0] + [len(a) for a in atoms_list])
    species = MS.species_of(atoms_list, ZS)
    return np.array([MS.record(x_hist[k], origin, masses, species, off, len(ZS), magnitudes) for k in range(every, len(x_hist), every)])


def _msd_error(got, want, scale):
    """The largest error of a record's sums, each relative to the sum of its terms' magnitudes."""
    return float((np.abs(got - want) / np.maximum(scale, 1e-300)).max())


def test_msd_records_of_the_crossing_run_equal_the_restatement_on_the_reference_trajectory():
    ref = MS.flight("fast", "wrapped")
    got = _flight("fast", 0.5, True, msd_every=5)
    rec = got["rec"]
    want = _msd_reference(ref["x_hist"], ref["x0"], 5, [MS.base()], ref["m"])
    assert rec["msd_sums"].shape == want.shape == (8, 1, 12) and list(rec["msd_step"]) == list(range(5, 45, 5))
    scale = _msd_reference(ref["x_hist"], ref["x0"], 5, [MS.base()], ref["m"], True)
    err = _msd_error(rec["msd_sums"], want, scale)
    cell = np.asarray(MS.base().get_cell(), float)
    w_end = float(rec["msd"][-1, 0, 1])
    print(f"msd sums against the restatement: {err:.2e} relative; W msd at the end {w_end:.2f} A^2 (half a cell squared: "
          f"{(0.5 * cell[0, 0]) ** 2:.2f}), Mo {rec['msd'][-1, 0, 0]:.4f}")
    assert err <= TOL
    assert w_end > 25.0 > (0.5 * cell[0, 0]) ** 2                # (a sampler that forgets the image counts cannot get there)
    # the derived entries are md.msd_records of those sums: checked against the direct formulas on the reference trajectory
    species, off = MS.species_of([MS.base()], ZS), np.array([0, 16])
    for k in range(8):
        msd, msd_all, com, com_all = MS.direct(ref["x_hist"][5 * (k + 1)], ref["x0"], ref["m"], species, off, 2)
        for key, val in (("msd", msd), ("msd_all", msd_all), ("msd_com_removed", com), ("msd_all_com_removed", com_all)):
            assert np.allclose(rec[key][k], val, rtol=TOL, atol=TOL * w_end), (key, k)


@pytest.mark.parametrize("wrap", [False, True])
def test_msd_sampling_leaves_the_trajectory_alone_and_repeats_bit_for_bit(wrap):
    plain, a, b = _flight("fast", 0.5, wrap), _flight("fast", 0.5, wrap, msd_every=5), _flight("fast", 0.5, wrap, (40,), 5)
    for k in ("x", "v", "e", "f"):
        assert np.array_equal(plain[k], a[k]), k
    for k in ("potential_energy", "kinetic_energy", "temperature", "step"):
        assert np.array_equal(plain["rec"][k], a["rec"][k]), k
    assert a is not b and np.array_equal(a["rec"]["msd_sums"], b["rec"]["msd_sums"])


def test_msd_of_an_object_that_does_not_wrap_equals_the_host_formula():
    frames = [MS.base(), RH.CASES["slab_mow"][0]]
    m = DC.masses_of(frames)
    off = np.cumsum([0] + [len(a) for a in frames])
    species = MS.species_of(frames, ZS)
    with _dynamics(frames, seed=3) as dyn:
        dyn.initialize_velocities(300.0)
        x0 = dyn.get_positions()
        first = dyn.run(10, msd_every=10)
        x10 = dyn.get_positions()
        # a given origin, and blocks: the origin stays, the steps go on counting
        dyn.set_msd_origin(x0 + 0.25)
        second = dyn.run(20, msd_every=20)
        x30 = dyn.get_positions()
        assert not dyn.get_images().any()
    for rec, x, origin, step in ((first, x10, x0, 10), (second, x30, x0 + 0.25, 30)):
        want = MS.record(x, origin, m, species, off, 2)
        err = _msd_error(rec["msd_sums"][0], want, MS.record(x, origin, m, species, off, 2, True))
        print(f"wrap=False, step {step}: msd sums against the host formula {err:.2e}")
        assert err <= TOL and list(rec["msd_step"]) == [step]
    assert first["msd_all"][0, 0] > 1e-4 and abs(second["msd_all"][0, 0] - 3 * 0.25 ** 2) < 0.1


def test_msd_sums_of_many_chunks_and_a_species_a_frame_lacks():
    """588 W atoms (three chunks of the 256-wide chunk table, the last one partly filled) next to the 16-atom Mo/W cell."""
    big = synthetic.lattice_frame("bcc", (7, 7, 6), 3.165, [74], seed=8)
    frames = [big, MS.base()]
    n = len(big)
    assert n == 588
    m = DC.masses_of(frames)
    with _dynamics(frames, seed=4, wrap=True) as dyn:
        dyn.initialize_velocities(300.0)
        origin = dyn.get_positions() + np.random.default_rng(9).normal(0, 1.0, (n + 16, 3))
        dyn.set_msd_origin(origin)
        rec = dyn.run(2, msd_every=2)
        x = dyn.get_positions()
    want = MS.record(x, origin, m, MS.species_of(frames, ZS), np.array([0, n, n + 16]), 2)
    err = _msd_error(rec["msd_sums"][0], want, MS.record(x, origin, m, MS.species_of(frames, ZS), np.array([0, n, n + 16]), 2, True))
    print(f"588 + 16 atoms: msd sums against the host formula {err:.2e}")
    assert err <= TOL
    assert np.isnan(rec["msd"][0, 0, 0]) and np.all(np.isfinite(rec["msd"][0, 1])) and np.isfinite(rec["msd"][0, 0, 1])


# =================================================================================================================== 6. left alone
def _mixed():
    return [_w128(1), _cluster(), RH.CASES["slab_mow"][0]]


def _mixed_run(wrap, touch=False):
    frames = _mixed()
    with _dynamics(frames, seed=2, wrap=wrap) as dyn:
        if touch:                       # (the new entries that leave a wrap=False object what it is)
            dyn.wrap = False
            assert not dyn.get_images().any()
            dyn.set_msd_origin()
        dyn.initialize_velocities(300.0)
        rec = dyn.run(30, thermo_every=5)
        return dict(_state(dyn), rec=rec, img=dyn.get_images())


def test_axes_that_are_not_periodic_and_objects_that_do_not_wrap_are_left_alone():
    frames = _mixed()
    assert [tuple(a.get_pbc()) for a in frames] == [(True,) * 3, (False,) * 3, (True, True, False)]
    off = np.cumsum([0] + [len(a) for a in frames])
    never, touched, wrapping = _mixed_run(False), _mixed_run(False, touch=True), _mixed_run(True)
    # a wrap=False object: bit for bit the object that never met the new entries
    for k in ("x", "v", "e", "f"):
        assert np.array_equal(never[k], touched[k]), k
    for k in never["rec"]:
        assert np.array_equal(never["rec"][k], touched["rec"][k]), k
    assert not never["img"].any()
    # wrap=True: the cluster and the slab's z are bit for bit those of the wrap=False run
    cluster, slab = slice(off[1], off[2]), slice(off[2], off[3])
    print(f"wrap=True: image counts of the bulk frame up to {np.abs(wrapping['img'][:off[1]]).max()}, of the slab up to "
          f"{np.abs(wrapping['img'][slab]).max()}")
    assert np.array_equal(wrapping["x"][cluster], never["x"][cluster])
    assert np.array_equal(wrapping["x"][slab, 2], never["x"][slab, 2])
    assert not wrapping["img"][cluster].any() and not wrapping["img"][slab, 2].any()


def test_the_wrap_kernel_leaves_non_periodic_axes_bit_for_bit():
    """Atoms given far outside their cells.  The stored positions of the cluster stay the bits given, and so do those of the
    slab's atoms that were moved along its third, non-periodic cell vector alone (every second one); the slab's other atoms
    are folded along the two periodic vectors only (whose z components, in this strained cell, are not zero), the bulk
    frame's along all three."""
    frames = _mixed()
    rng = np.random.default_rng(12)
    given = []
    for k, a in enumerate(frames):
        cell = np.asarray(a.get_cell(), float)
        n = rng.integers(-3, 4, (len(a), 3))
        n[n == 0] = 2
        if k == 2:
            n[::2, :2] = 0
        given.append(a.get_positions() + n @ cell)
    moved = [Atoms(numbers=a.get_atomic_numbers(), positions=x, cell=a.get_cell(), pbc=a.get_pbc()) for a, x in zip(frames, given)]
    off = np.cumsum([0] + [len(a) for a in frames])
    with _dynamics(moved, wrap=True) as dyn:
        stored = np.empty((off[-1], 3))
        img = np.empty((off[-1], 3), dtype=np.int32)
        dyn.ctx.check(dyn.ctx.lib.uf3_md_get_wrapped(dyn._live(), _lib._p(stored), _lib._p(img)))
        x = dyn.get_positions()
    g = np.concatenate(given)
    assert np.array_equal(stored[off[1]:off[2]], g[off[1]:off[2]]) and not img[off[1]:off[2]].any()
    assert np.array_equal(stored[off[2]::2], g[off[2]::2]) and not img[off[2]::2].any() and not img[off[2]:, 2].any()
    assert _inside(stored[:off[1]], frames[0].get_cell()) and _inside(stored[off[2]:], frames[2].get_cell(), (True, True, False))
    # the image counts are the floors of the given fractional coordinates, against the cell (numpy's, on the host)
    assert np.array_equal(img[:off[1]], MS.images_of(given[0], np.asarray(frames[0].get_cell(), float)))
    assert np.array_equal(img[off[2]:, :2], MS.images_of(given[2], np.asarray(frames[2].get_cell(), float))[:, :2])
    assert np.abs(img[:off[1]]).max() >= 3 and np.abs(img[off[2] + 1::2, :2]).max() >= 3
    assert np.abs(x - g).max() <= 1e-12 * np.abs(g).max()


# ================================================================================================================== 7. skewed cell
def test_wrapping_takes_fractional_coordinates_against_a_skewed_cell():
    atoms = DC.get_pair("bcc_mow", "skew_821").atoms
    cell = np.asarray(atoms.get_cell(), float)
    assert np.abs(cell - np.diag(np.diag(cell))).max() > 1.0       # (skewed: edge lengths are not heights)
    x = atoms.get_positions().copy()
    x[6] += cell[1] - cell[0]
    moved = Atoms(numbers=atoms.get_atomic_numbers(), positions=x, cell=cell, pbc=True)
    vel = DC.velocities("bcc_mow", "skew_821")
    r = {}
    for key, a in (("unmoved", atoms), ("moved", moved)):
        with _dynamics([a], vel, wrap=True) as dyn:
            img0 = dyn.get_images()
            r[key] = dict(rec=dyn.run(30, thermo_every=1), img0=img0, wrapped=dyn.get_positions(wrap=True), x=dyn.get_positions())
    assert not r["unmoved"]["img0"].any() and list(r["moved"]["img0"][6]) == [-1, 1, 0] and np.abs(r["moved"]["img0"]).sum() == 2
    d = float(np.abs(r["moved"]["rec"]["potential_energy"] - r["unmoved"]["rec"]["potential_energy"]).max())
    dx = float(np.abs(r["moved"]["x"] - r["unmoved"]["x"] - (x - atoms.get_positions())).max())
    print(f"skew_821, one atom moved by a lattice vector: energies of 30 NVE steps differ by {d:.2e} eV, positions by {dx:.2e} A")
    assert d <= TOL and dx <= TOL
    assert _inside(r["moved"]["wrapped"], cell)


# ========================================================================================================= 8. blocks and switches
def test_blocks_agree_with_one_run_to_rounding():
    one, two = _flight("fast", 0.5, True), _flight("fast", 0.5, True, (15, 25))
    fig = _figures(two, one)
    print(f"[40] against [15, 25] on the crossing run: {fig}")
    assert max(fig.values()) <= BLOCK_TOL
    assert np.array_equal(one["img"], two["img"])


def test_switching_wrap_off_and_setting_positions():
    x0, v0, m = MS.start("fast")
    cell = np.asarray(MS.base().get_cell(), float)
    with _dynamics([MS.base()], v0, wrap=True) as dyn:
        dyn.run(20)
        assert dyn.get_images()[MS.ATOM].any()
        x, e = dyn.get_positions(), dyn.get_potential_energies()
        dyn.wrap = False
        assert dyn.wrap is False and not dyn.get_images().any()
        assert np.abs(dyn.get_positions() - x).max() <= 1e-12
        # (the object now follows the default rule: the energy of the unwrapped positions is another one)
        assert abs(dyn.get_potential_energies()[0] - e[0]) > 1e-3
        dyn.wrap = True
        assert dyn.get_images()[MS.ATOM].any() and np.abs(dyn.get_positions() - x).max() <= 1e-12
        assert abs(dyn.get_potential_energies()[0] - e[0]) <= TOL * abs(e[0])
        # set_positions: as given, images zero; the next evaluation wraps again
        given = x0 + np.array([2, -1, 0]) @ cell
        dyn.set_positions(given)
        assert not dyn.get_images().any() and np.array_equal(dyn.get_positions(), given)
        dyn.get_forces()
        assert np.array_equal(dyn.get_images(), np.tile([2, -1, 0], (16, 1)))
        assert np.abs(dyn.get_positions() - given).max() <= 1e-12


# ================================================================================================================ 9. the ABI's checks
def test_the_new_entries_check_their_arguments_under_their_own_names():
    lib = _ctx().lib
    null = C.c_void_p()
    buf = np.zeros((4, 1, 12))
    run = (10, 1.0, 0.0, 0.0, 0, 0.5, 0, 0, None)

    def message():
        return lib.uf3_last_error(_ctx().handle).decode()
    for call in (lambda: lib.uf3_md_set_wrap(null, 1), lambda: lib.uf3_md_get_wrapped(null, None, None),
                 lambda: lib.uf3_md_msd_origin(null, None), lambda: lib.uf3_md_run_msd(null, *run, 5, _lib._p(buf))):
        assert call() == 1
    with _dynamics([MS.base()]) as dyn:
        h = dyn._live()
        for args, text in (((*run, -1, None), "uf3_md_run_msd: msd_every must be >= 0"),
                           ((*run, 5, None), "uf3_md_run_msd: msd records are due but the msd buffer is NULL"),
                           ((*run, 0, _lib._p(buf)), "uf3_md_run_msd: a msd buffer was given but no record is due"),
                           ((*run, 20, _lib._p(buf)), "uf3_md_run_msd: a msd buffer was given but no record is due"),
                           ((-1, *run[1:], 0, None), "uf3_md_run_msd: n_steps must be >= 0"),
                           ((10, 0.0, *run[2:], 0, None), "uf3_md_run_msd: dt must be positive and finite"),
                           ((*run[:5], 9.0, *run[6:], 0, None), "uf3_md_run_msd: skin must lie in [0, 4] Angstrom"),
                           ((*run[:6], 5, 0, None, 0, None), "uf3_md_run_msd: thermo records are due but the thermo buffer is NULL")):
            assert lib.uf3_md_run_msd(h, *args) == 1, text
            assert message() == text
        bad = np.full((16, 3), np.nan)
        assert lib.uf3_md_msd_origin(h, _lib._p(bad)) == 1 and message() == "uf3_md_msd_origin: origin must be finite"
        assert dyn.step == 0
        # at a pressure, and next to another sampler: refused under the entry's name before anything runs
        with pytest.raises(_lib.UF3Error, match="uf3_md_run_msd: msd_every does not go into one run"):
            dyn.run(10, msd_every=5, flux_every=5)
        with pytest.raises(ValueError, match="MolecularDynamics: positions must be"):
            dyn.set_msd_origin(np.zeros((3, 3)))
    with _dynamics([MS.base()], temperature_K=300.0, pressure_eV_A3=0.0, barostat_time_fs=500.0) as dyn:
        with pytest.raises(_lib.UF3Error, match="uf3_md_run_msd: .*constant volume only"):
            dyn.run(10, msd_every=5)
        assert dyn.step == 0
