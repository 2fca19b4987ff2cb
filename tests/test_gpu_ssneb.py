"""Nudged elastic bands with changing cells on the device (``uf3_ssneb_create``, ``neb.CellNudgedElasticBand``) against the NumPy
restatement in tests/_ssneb_ref.py, whose energies, forces and strain derivatives come from ``UFCalculator.evaluate_frames``:
step-by-step parity with and without a climbing image, the generalised force as the energy's gradient, a converged
lattice-invariant shear of bcc W, batch independence, cadence and split invariance, freezing, refusals, records, the context
left as it was found, and the positions-only band unchanged."""
import ctypes as C
import functools

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator, neb
from uf3_amd.forcefield.neb import CellNudgedElasticBand, NudgedElasticBand
import _ssneb_ref as S
from test_gpu_neb import A0_W, MARGIN, STATUS, TOL, _hop, _mow, _unary
from test_gpu_redescribed import FD_H, FD_TOL

pytestmark = pytest.mark.gpu
OFFSET = 0.0625         # fractional: every atom starts inside its cell and stays there (the evaluator's image range)


def _bcc(reps, a=A0_W, numbers=(74,), seed=0):
    grid = np.stack(np.meshgrid(*[np.arange(r) for r in reps], indexing="ij"), axis=-1).reshape(-1, 1, 3)
    frac = ((grid + np.array([[0, 0, 0], [.5, .5, .5]])[None]).reshape(-1, 3)) / np.array(reps, float) + OFFSET / np.array(reps, float)
    z = np.random.default_rng(seed).choice(np.asarray(numbers), len(frac)) if len(numbers) > 1 else np.full(len(frac), numbers[0])
    return frac, np.diag(np.array(reps, float) * a), z


def _end(frac, cell, z, seed, rattle, strain=0.0):
    """The crystal in ``cell`` strained by a seeded matrix (shear included), atoms rattled."""
    rng = np.random.default_rng(seed)
    c = cell @ (np.eye(3) + rng.uniform(-strain, strain, (3, 3)))
    return Atoms(numbers=z, positions=frac @ c + rng.normal(0, rattle, frac.shape), cell=c, pbc=True)


def _strained_band(m, reps, seed, strain=(0.0, 0.03), a=A0_W, numbers=(74,), push=None):
    """m images between two strained, independently rattled (0.002 / 0.005 Angstrom: tests/test_gpu_neb.py's _hop) descriptions
    of bcc; ``push``: atom 3 of the last image is displaced by it (a band whose images differ although their cells do not)."""
    frac, cell, z = _bcc(reps, a, numbers, seed)
    ini, fin = _end(frac, cell, z, seed, 0.002, strain[0]), _end(frac, cell, z, seed + 1000, 0.005, strain[1])
    if push is not None:
        fin.positions[3] += push
    return neb.interpolate(ini, fin, m, interpolate_cell=True)


def _batches():
    return {"w_cells": (_unary, lambda: [_strained_band(5, (2, 2, 2), 3), _strained_band(3, (3, 3, 3), 5, strain=(0.01, 0.04)),
                                         _strained_band(4, (5, 5, 6), 7, strain=(0.0, 0.02)),
                                         _strained_band(4, (2, 2, 2), 9, strain=(0.0, 0.0), push=[0.25, 0.1, -0.15])]),
            "mow54": (_mow, lambda: [_strained_band(6, (3, 3, 3), 11, strain=(0.01, 0.04), a=3.2, numbers=(42, 74))])}


def _reference(calc, bands, **kw):
    frames = [a for b in bands for a in b]
    off = np.cumsum([0] + [len(a) for a in frames])

    def evaluate(x, cells):
        moved = [Atoms(numbers=a.get_atomic_numbers(), positions=x[off[k]:off[k + 1]], cell=cells[k], pbc=True)
                 for k, a in enumerate(frames)]
        e, f, _, w = calc.evaluate_frames(moved, virial=True)
        return e, f, w
    x0 = np.concatenate([a.get_positions() for a in frames])
    cells = np.array([np.asarray(a.get_cell(), dtype=float) for a in frames])
    return S.CellBand(evaluate, x0, cells, off, np.cumsum([0] + [len(b) for b in bands]), **kw)


def test_the_batches_hold_what_they_should():
    bands = _batches()["w_cells"][1]()
    assert [(len(b), len(b[0])) for b in bands] == [(5, 16), (3, 54), (4, 300), (4, 16)]
    assert not np.allclose(np.asarray(bands[0][0].get_cell()), np.asarray(bands[0][-1].get_cell()))
    assert np.array_equal(np.asarray(bands[3][0].get_cell()), np.asarray(bands[3][-1].get_cell()))
    shear = np.linalg.inv(np.asarray(bands[0][0].get_cell())) @ np.asarray(bands[0][-1].get_cell())
    assert np.abs(shear - np.diag(np.diag(shear))).max() > 1e-3
    for b in bands:
        for a in b:
            s = a.get_positions() @ np.linalg.inv(np.asarray(a.get_cell()))
            assert s.min() > 0.0 and s.max() < 1.0
    assert [(len(b), len(b[0])) for b in _batches()["mow54"][1]()] == [(6, 54)]


@pytest.mark.parametrize("climb", [False, True], ids=["plain", "climb"])
@pytest.mark.parametrize("name", ["w_cells", "mow54"])
def test_parity_with_the_restatement(name, climb):
    make_calc, make_bands = _batches()[name]
    calc, bands = make_calc(), make_bands()
    nb = len(bands)
    spring = np.linspace(0.1, 0.3, nb)
    kappa = np.array([float(len(b[0])) * (1.0 + 0.5 * k) for k, b in enumerate(bands)])
    ref = _reference(calc, bands, spring=spring, cell_factor=kappa)
    fmax, kw = 1e-3, dict(climb=climb, dt=0.1, dt_max=1.0, maxstep=0.2)
    worst = [0.0, 0.0, 0.0]
    with CellNudgedElasticBand(calc, bands, spring=spring, cell_factor=kappa) as band:
        for k in range(30):
            out = band.run(1, fmax=fmax, **kw)
            ref.run(1, fmax=fmax, **kw)
            x, cells = band.get_positions(), band.get_cells()
            e = np.concatenate(out["energies"])
            d = [np.abs(x - ref.x).max(), np.abs(e - ref.e_last).max(), np.abs(cells - ref.cells).max()]
            worst = [max(a, b) for a, b in zip(worst, d)]
            assert d[0] <= TOL and d[2] <= TOL, (k, d)
            assert d[1] <= TOL, (k, e, ref.e_last)
            assert out["climbing_image"].tolist() == ref.climbing.tolist()
            assert np.abs(out["criterion"] - ref.crit).max() <= 1e-8
        assert np.abs(band.get_neb_forces() - ref.g).max() <= 1e-8 and np.abs(band.get_neb_cell_forces() - ref.gc).max() <= 1e-8
        assert np.abs(band.get_forces() - ref.fq).max() <= 1e-8 and np.abs(band.get_cell_forces() - ref.G).max() <= 1e-8
        print(f"ssneb parity {name} climb={climb}: 30 steps dx {worst[0]:.3g} dE {worst[1]:.3g} dcell {worst[2]:.3g}; "
              f"smallest margin {min(ref.margins):.3g} eV; steps {ref.steps.tolist()} status {ref.status.tolist()}; "
              f"|power| >= {np.abs(ref.power).min():.3g}")
        # the condition on the inputs: no energy ordering the restatement branched on was closer than MARGIN
        assert min(ref.margins) >= MARGIN, (min(ref.margins), int(np.argmin(ref.margins)))
        assert out["status"] == [STATUS[s] for s in ref.status]
        assert out["steps"].tolist() == ref.steps.tolist()
        assert ref.max_dr <= 0.2 * (1 + 1e-12)
        # the interior cells moved, also in the band whose end cells are equal; end cells were never written
        c0 = np.array([np.asarray(a.get_cell()) for b in bands for a in b])
        first = band.band_first
        for b in range(nb):
            assert np.array_equal(cells[first[b]], c0[first[b]]) and np.array_equal(cells[first[b + 1] - 1], c0[first[b + 1] - 1])
            assert np.abs(cells[first[b] + 1:first[b + 1] - 1] - c0[first[b] + 1:first[b + 1] - 1]).max() > 1e-6


def test_the_generalised_force_is_the_gradient():
    """Central differences of ``evaluate_frames`` energies along seeded (q, Y) directions: tests/test_gpu_redescribed.py's
    Richardson pair and tolerance (FD_TOL of the largest entry of the force)."""
    calc = _unary()
    band = _strained_band(3, (2, 2, 2), 21, strain=(0.02, 0.05))
    band[1].positions += np.random.default_rng(4).normal(0, 0.03, (16, 3))
    kap = 7.5
    with CellNudgedElasticBand(calc, band, cell_factor=kap) as b:
        FF = np.concatenate([b.get_forces()[16:32], b.get_cell_forces()[1]])
    c0 = np.asarray(band[0].get_cell())
    D = np.linalg.inv(c0) @ np.asarray(band[1].get_cell())
    q, Y = band[1].get_positions() @ np.linalg.inv(D), kap * D

    def energy(q, Y):
        d = Y / kap
        return calc.evaluate_frames([Atoms(numbers=band[1].get_atomic_numbers(), positions=q @ d, cell=c0 @ d, pbc=True)], forces=False)[0][0]
    rng = np.random.default_rng(22)
    for _ in range(6):
        u = rng.normal(0, 1, (19, 3))
        u /= np.sqrt(np.vdot(u, u))
        d = [-(energy(q + h * u[:16], Y + h * u[16:]) - energy(q - h * u[:16], Y - h * u[16:])) / (2 * h) for h in FD_H]
        fd = (4 * d[1] - d[0]) / 3
        assert abs(fd - np.vdot(FF, u)) <= FD_TOL * np.abs(FF).max(), (fd, np.vdot(FF, u))


def _shear_ends():
    """bcc W 2 x 2 x 2 and the same crystal described in the cell whose first row is shifted by the lattice vector a e_y; every
    atom goes to the nearest site of that description, and all stay inside their cells along the way."""
    frac, cell, z = _bcc((2, 2, 2))
    sheared = cell.copy()
    sheared[0] += 0.5 * cell[1]
    s1 = frac @ cell @ np.linalg.inv(sheared)                          # the same positions: s1[:, 1] = s[:, 1] - s[:, 0] / 2
    w = np.mod(s1[:, 1] - frac[:, 1], 0.5)                             # (a e_y is half a cell row: sites repeat every 1/2)
    s1[:, 1] = frac[:, 1] + np.where(w > 0.25, w - 0.5, w)
    assert s1.min() > 0.0 and s1.max() < 1.0
    return (Atoms(numbers=z, positions=frac @ cell, cell=cell, pbc=True), Atoms(numbers=z, positions=s1 @ sheared, cell=sheared, pbc=True))


@functools.lru_cache(None)
def _converged():
    calc = _unary()
    ends, info = calc.relax_frames(list(_shear_ends()), fmax=1e-5, relax_cell=True, max_steps=2000)
    assert np.all(info["converged"])
    band = neb.interpolate(ends[0], ends[1], 7, mic=False, interpolate_cell=True)
    bands, info = calc.neb_bands([band, band[::-1]], fmax=2e-3, climb=True, max_steps=4000, relax_cell=True)
    return calc, bands, info


def test_a_lattice_invariant_shear_converges():
    calc, bands, info = _converged()
    fmax = 2e-3
    assert info["status"] == ["converged"] * 2, (info["status"], info["criterion"])
    band, ci = bands[0], int(info["climbing_image"][0])
    e, f, off, w = calc.evaluate_frames(band, virial=True)
    assert np.abs(e - info["energies"][0]).max() <= 1e-9
    assert 0 < ci < 6 and ci == int(np.argmax(e))
    steps = int(info["steps"].max())
    print(f"bcc W lattice-invariant shear (16 atoms, 7 images): barrier {info['barrier'][0]:.6f} eV, reverse "
          f"{info['reverse_barrier'][0]:.6f} eV, reversed band {info['barrier'][1]:.6f} eV, steps {info['steps'].tolist()}, "
          f"climbing image {ci}, energies {np.round(e - e[0], 6).tolist()}")
    assert info["barrier"][0] > 0
    assert abs(info["barrier"][0] - info["reverse_barrier"][0]) <= TOL * max(steps, 1)       # the same crystal at both ends
    assert abs(info["barrier"][1] - info["barrier"][0]) <= 1e-4                             # (tests/test_gpu_neb.py's hop)
    # the climbing image: |g| = |F| over the whole vector, and every row of g is below fmax
    n = len(band[0])
    D = np.linalg.inv(np.asarray(band[0].get_cell())) @ np.asarray(band[ci].get_cell())
    FF = np.concatenate([f[off[ci]:off[ci + 1]] @ D.T, -(np.linalg.inv(D).T @ S.voigt_to_matrix(w[ci])) / n])
    assert np.sqrt(np.vdot(FF, FF)) < fmax * np.sqrt(n + 3)
    # interior cells differ from the interpolated ones: the cell was a degree of freedom
    assert all(np.all(a.get_pbc()) for a in band)


def test_bands_behave_alike_alone_and_in_a_batch():
    calc = _unary()
    bands = _batches()["w_cells"][1]()
    kw = dict(fmax=1e-3, climb=True)
    kappa = [16.0, 80.0, 300.0, 24.0]
    with CellNudgedElasticBand(calc, bands, cell_factor=kappa) as band:
        batch = band.run(60, **kw)
        xb, cb = band.get_positions(), band.get_cells()
    lo = f = 0
    for k, b in enumerate(bands):
        n = len(b) * len(b[0])
        with CellNudgedElasticBand(calc, b, cell_factor=kappa[k]) as band:
            alone = band.run(60, **kw)
            x, c = band.get_positions(), band.get_cells()
        assert alone["status"][0] == batch["status"][k] and alone["steps"][0] == batch["steps"][k]
        assert alone["climbing_image"][0] == batch["climbing_image"][k]
        assert np.abs(x - xb[lo:lo + n]).max() <= 1e-8 and np.abs(c - cb[f:f + len(b)]).max() <= 1e-8
        lo += n
        f += len(b)


def test_cadence_and_splitting_do_not_change_the_result():
    calc = _unary()
    bands = [_strained_band(5, (2, 2, 2), 3), _strained_band(3, (3, 3, 3), 5, strain=(0.01, 0.04))]
    kw = dict(fmax=1e-3, climb=True)
    finals = []
    for every in (1, 50):
        with CellNudgedElasticBand(calc, bands) as band:
            out = band.run(100, check_every=every, **kw)
            finals.append((band.get_positions(), band.get_cells(), out["status"], out["steps"], np.concatenate(out["energies"])))
    (x1, c1, s1, n1, e1), (x2, c2, s2, n2, e2) = finals
    assert np.array_equal(x1, x2) and np.array_equal(c1, c2) and s1 == s2 and np.array_equal(n1, n2) and np.array_equal(e1, e2)
    with CellNudgedElasticBand(calc, bands) as band:
        band.run(37, **kw)
        out = band.run(63, **kw)
        assert out["status"] == s1 and np.array_equal(out["steps"], n1)
        assert np.abs(band.get_positions() - x1).max() <= 1e-10 and np.abs(band.get_cells() - c1).max() <= 1e-10


def test_a_non_finite_cell_force_freezes_only_its_band():
    """The library and the class refuse non-finite positions at creation, as ``uf3_neb_create`` does, so no NaN position can
    reach the device (tests/test_ssneb_host.py puts one into the restatement).  The smallest positive ``cell_factor`` is
    finite and passes every check, and makes the cell force -D^-T W / kappa overflow at the first evaluation: that band
    ends ``nonfinite`` without a move, the other bands do not notice."""
    calc = _unary()
    bad, other = _strained_band(4, (2, 2, 2), 9, strain=(0.0, 0.03)), _strained_band(5, (2, 2, 2), 3)
    x0 = np.concatenate([a.get_positions() for a in bad])
    with CellNudgedElasticBand(calc, [bad, other], cell_factor=[5e-324, 16.0]) as band:
        out = band.run(20, fmax=1e-3, climb=True)
        x, cells = band.get_positions(), band.get_cells()
    assert out["status"][0] == "nonfinite" and out["steps"][0] == 0 and np.isnan(out["criterion"][0])
    assert out["climbing_image"][0] == -1 and np.array_equal(x[:len(x0)], x0)
    assert np.array_equal(cells[:4], np.array([np.asarray(a.get_cell()) for a in bad]))
    assert np.all(np.isfinite(out["energies"][0]))
    with CellNudgedElasticBand(calc, other) as band:
        alone = band.run(20, fmax=1e-3, climb=True)
        xa, ca = band.get_positions(), band.get_cells()
    assert out["status"][1] == alone["status"][0] and out["steps"][1] == alone["steps"][0] > 0
    assert np.abs(x[len(x0):] - xa).max() <= 1e-8 and np.abs(cells[4:] - ca).max() <= 1e-8


def _with(band, j, **kw):
    a = band[j]
    args = dict(numbers=a.get_atomic_numbers(), positions=a.get_positions(), cell=a.get_cell(), pbc=a.get_pbc())
    args.update(kw)
    out = list(band)
    out[j] = Atoms(**args)
    return out


def test_the_class_refuses_before_the_device_is_touched(monkeypatch):
    calc = _unary()
    band = _strained_band(4, (2, 2, 2), 9)

    def refuse(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "get_context", refuse)
    z = band[2].get_atomic_numbers().copy()
    z[4] = 42
    flat = np.asarray(band[1].get_cell()).copy()
    flat[2] = flat[1]
    for kw, match in ((dict(bands=[Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions(), cell=a.get_cell(),
                                         pbc=[True, True, False]) for a in band]), "periodic along all three"),
                      (dict(bands=_with(band, 1, cell=flat)), "singular"), (dict(bands=_with(band, 2, numbers=z)), "species"),
                      (dict(cell_factor=0.0), "cell_factor"), (dict(cell_factor=-2.0), "cell_factor"),
                      (dict(cell_factor=[16.0, 16.0]), "cell_factor")):
        args = dict(calc=calc, bands=band)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            CellNudgedElasticBand(**args)
    with pytest.raises(TypeError, match="fixed"):
        CellNudgedElasticBand(calc, band, fixed=np.zeros(64, bool))
    with pytest.raises(ValueError, match="fixed"):
        calc.neb_bands(band, relax_cell=True, fixed=np.zeros(64, bool))


def _create(calc, band_lists, edit=None, cell_factor=None, plain=False):
    """uf3_ssneb_create (``plain``: uf3_neb_create) on the raw ABI; returns (rc, message, handle or None)."""
    batch = _lib.FrameBatch([a for b in band_lists for a in b])
    if edit:
        edit(batch)
    first = np.ascontiguousarray(np.cumsum([0] + [len(b) for b in band_lists]), dtype=np.int32)
    spring = np.full(len(band_lists), 0.1)
    ctx = _lib.get_context(calc.device)
    db = _lib.device_basis(calc.bspline_config, ctx)
    h = C.c_void_p()
    model = [_lib._p(calc._c1), _lib._p(calc._c2), _lib._p(calc._c3)]
    if plain:
        rc = ctx.lib.uf3_neb_create(db.handle, C.byref(batch.struct), _lib._p(batch.pos), _lib._p(batch.z), None, *model,
                                    len(band_lists), _lib._p(first), _lib._p(spring), C.byref(h))
    else:
        cf = None if cell_factor is None else np.asarray(cell_factor, dtype=float)
        rc = ctx.lib.uf3_ssneb_create(db.handle, C.byref(batch.struct), _lib._p(batch.pos), _lib._p(batch.z), *model,
                                      len(band_lists), _lib._p(first), _lib._p(spring), _lib._p(cf), C.byref(h))
    return rc, ctx.lib.uf3_last_error(ctx.handle).decode(), (h if rc == 0 else None), ctx


def test_the_library_refuses_bad_cell_bands():
    calc = _unary()
    band = _strained_band(4, (2, 2, 2), 9)
    rc, _, h, ctx = _create(calc, [band])                              # cell_factor NULL: the atom count
    assert rc == 0
    ctx.lib.uf3_neb_destroy(h)

    def species(batch):
        batch.z[16 + 4] = 42

    def pbc(batch):
        batch.pbc[:, 2] = 0

    def singular(batch):
        batch.cells[2, 1] = batch.cells[2, 0]

    def same(batch):
        batch.pos[32:48] = batch.pos[16:32]
    for edit, match in ((species, "species"), (pbc, "periodic along all three"), (singular, "singular"), (same, "identical to image 1")):
        rc, msg = _create(calc, [_strained_band(4, (2, 2, 2), 9)], edit=edit)[:2]     # (a fresh band: the batch shares its arrays)
        assert rc == 1 and match in msg, (match, msg)
    rc, msg = _create(calc, [band, band[:2]])[:2]
    assert rc == 1 and "band 1 has 2 images" in msg
    for bad in (0.0, -1.0, np.inf, np.nan):
        rc, msg = _create(calc, [band], cell_factor=[bad])[:2]
        assert rc == 1 and "cell_factor" in msg, bad
    # uf3_neb_create keeps refusing cells that differ, and so does the class
    rc, msg = _create(calc, [band], plain=True)[:2]
    assert rc == 1 and "cell differs" in msg
    with pytest.raises(ValueError, match="cell differs"):
        NudgedElasticBand(calc, band)


def test_the_cell_state_of_a_plain_handle_is_refused():
    calc = _unary()
    with NudgedElasticBand(calc, _hop(4, 9, reps=(2, 2, 2))) as band:
        cells = np.zeros((4, 3, 3))
        assert band.ctx.lib.uf3_neb_get_cell_state(band.handle, _lib._p(cells), None, None, None) == 1
        assert "not a cell band" in band.ctx.lib.uf3_last_error(band.ctx.handle).decode()
    with CellNudgedElasticBand(calc, _strained_band(4, (2, 2, 2), 9)) as band:
        assert band.ctx.lib.uf3_neb_get_cell_state(band.handle, None, None, None, None) == 0
        w = band.get_virials()
        e, f, _, w0 = calc.evaluate_frames(band.get_images(), virial=True)
        assert np.abs(w - w0).max() <= 1e-9 and np.all(band.get_neb_cell_forces()[[0, 3]] == 0.0)


def test_records_follow_the_run():
    calc = _unary()
    ends, info = calc.relax_frames(list(_shear_ends()), fmax=1e-5, relax_cell=True, max_steps=2000)
    bands = [neb.interpolate(ends[0], ends[1], 7, mic=False, interpolate_cell=True), _strained_band(5, (2, 2, 2), 3)]
    with CellNudgedElasticBand(calc, bands) as band:
        out = band.run(600, fmax=5e-2, climb=True, record_every=10)
    rec = out["records"]
    assert rec["energies"].shape == (61, 12) and rec["criterion"].shape == (61, 2) and rec["iteration"][:3].tolist() == [0, 10, 20]
    assert out["status"] == ["converged"] * 2                              # (so the last rows repeat the final values)
    assert np.abs(rec["energies"][-1] - np.concatenate(out["energies"])).max() <= TOL
    assert np.array_equal(rec["criterion"][-1], out["criterion"])
    assert np.array_equal(rec["climbing_image"][-1], out["climbing_image"])
    assert np.array_equal(rec["energies"][-1], rec["energies"][-2]) and np.all(rec["criterion"][0] > rec["criterion"][-1])
    # end points never move: their energies are the same in every row
    assert np.abs(rec["energies"][:, [0, 6, 7, 11]] - rec["energies"][0, [0, 6, 7, 11]]).max() <= TOL


def test_runs_leave_the_context_as_they_found_it():
    """The run puts the context's MD skin to 0 and the caller's back, also when it fails: afterwards a calculator that keeps
    lists (skin 0.7, set before the runs) still finds the MD route -- its evaluations count as MD steps."""
    calc = _unary()
    keeper = calculator.UFCalculator(calc.model, md_skin=0.7)
    ctx = _lib.get_context(calc.device)
    other = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=61)
    band = _strained_band(4, (2, 2, 2), 9)
    try:
        e0, f0, _ = keeper.evaluate_frames([other])                        # (the context's skin is 0.7 from here on)
        steps0 = ctx.md_stats()["steps"]
        with CellNudgedElasticBand(calc, band) as b:
            b.run(5, fmax=1e-3, climb=True)
        assert ctx.md_stats()["steps"] == steps0                          # (the run itself: skin 0, no MD step)
        foreign = [Atoms(numbers=[42] * 3 + [74] * 13, positions=a.get_positions(), cell=a.get_cell(), pbc=True) for a in band]
        b = CellNudgedElasticBand(calc, foreign)
        with pytest.raises(_lib.SpeciesError):                             # Mo: outside the unary basis
            b.run(3)
        b.close()
        assert ctx.md_stats()["steps"] == steps0 and getattr(ctx, "_md_skin", 0.0) == 0.7
        e1, f1, _ = keeper.evaluate_frames([other])
        e2, f2, _ = keeper.evaluate_frames([other])
        assert ctx.md_stats()["steps"] == steps0 + 2
        assert np.array_equal(e0, e1) and np.array_equal(f0, f1) and np.array_equal(e1, e2)
    finally:
        ctx.md_skin(0.0)


def test_the_plain_band_is_unchanged():
    calc = _unary()
    band = _hop(5, 3)
    with NudgedElasticBand(calc, band) as b:
        b.run(40, fmax=1e-3, climb=False)
        b.run(0, fmax=1e-3, climb=True)
        x = b.get_positions()
    with pytest.warns(RuntimeWarning, match="did not converge"):
        images, info = calc.neb_bands(band, fmax=1e-3, max_steps=40, relax_cell=False)
    assert info["steps"].tolist() == [40]
    assert np.array_equal(np.concatenate([a.get_positions() for a in images]), x)
