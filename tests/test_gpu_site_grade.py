"""Site rows and extrapolation grades on the device (uf3_site_rows, uf3_site_grade, uf3_md_run_grade).

Rows: against the host rows of tests/_site_rows_ref.py (held to _flux_ref and the oracle by tests/test_site_rows_host.py), entry
by entry within 1e-10 of the largest |B| -- the bound the project holds U to (tests/test_gpu_flux.py).
Grades: against ``ls.leverage_reference`` of the DEVICE's rows within ``ls.leverage_bound``, the derived summation-order bound of
tests/test_gpu_leverage.py: the fused kernel, the fall-back and uf3_leverage add the same products in different orders.
Every test that means a route asserts it from the launch report (UF3_DEBUG_LDS, "uf3: site grade kernel=...")."""
import ctypes as C
import functools
import gc
import os
import re

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator
from uf3_amd.forcefield.md import MolecularDynamics
from uf3_amd.regression import least_squares as ls
from uf3_amd.representation import process
import _site_rows_ref as SR
from _bases import wide_basis as _wide_basis
from _util import GOLDEN, wrapped

pytestmark = pytest.mark.gpu

RTOL = 1e-10
TILE = 16                        # SG_TILE, uf3_amd/csrc/uf3_site_rows.h
CASES = ["unary", "mow", "uneven", "sym1", "cluster", "pairs"]


# ------------------------------------------------------------------------------------------------ plumbing
def _dev(basis):
    ctx = _lib.get_context(None)
    return ctx, _lib.device_basis(basis, ctx)


def _rows(basis, frames, ld=None, fill=None):
    ctx, db = _dev(basis)
    batch = _lib.FrameBatch(list(frames))
    ld = db.n_feat if ld is None else ld
    rows = np.empty((batch.n_atoms, ld))
    if fill is not None:
        rows[:] = fill
    ctx.check(ctx.lib.uf3_site_rows(db.handle, C.byref(batch.struct), _lib._p(batch.pos), _lib._p(batch.z), _lib._p(rows), ld))
    return rows


def _grades(basis, frames, w):
    ctx, db = _dev(basis)
    batch = _lib.FrameBatch(list(frames))
    w = np.ascontiguousarray(w, dtype=np.float64)
    assert w.shape == (db.n_feat, db.n_feat)
    g, fm, fa = np.empty(batch.n_atoms), np.empty(batch.n_frames), np.empty(batch.n_frames, dtype=np.int32)
    ctx.check(ctx.lib.uf3_site_grade(db.handle, C.byref(batch.struct), _lib._p(batch.pos), _lib._p(batch.z), _lib._p(w), _lib._p(g),
                                     _lib._p(fm), _lib._p(fa)))
    return g, fm, fa


@functools.lru_cache(maxsize=None)
def _w(name):
    w = SR.seeded_model(SR.case(name)[0]).whitening()
    w.setflags(write=False)
    return w


@pytest.fixture
def report(monkeypatch, capfd):
    """A fresh context that reports its launches; ``report()`` returns (and clears) the kernels of the site-grade launches
    since the last look."""
    monkeypatch.setenv("UF3_DEBUG_LDS", "1")
    monkeypatch.setattr(_lib, "_contexts", {})

    def drop():          # (device tables belong to the context they were made on: none from before, none left behind)
        for basis in [SR.case(name)[0] for name in CASES] + [_wide_basis()]:
            _lib.drop_device_basis(basis)
        gc.collect()

    def read():
        err = capfd.readouterr().err
        return [dict(kv.split("=") for kv in m.group(1).split() if "=" in kv)
                for m in re.finditer(r"uf3: site grade (.*)", err)]
    drop()
    yield read
    drop()


def _w16():
    return SR.case("unary")[1]


def _sub(atoms, n):
    """the first n atoms of a frame, its cell kept"""
    return Atoms(numbers=np.asarray(atoms.get_atomic_numbers())[:n], positions=np.asarray(atoms.get_positions())[:n],
                 cell=atoms.get_cell(), pbc=atoms.get_pbc())


def _w1():
    return Atoms(numbers=[74], positions=[[0.3, 0.1, 0.2]], cell=np.diag([3.165, 3.2, 3.1]), pbc=True)


# ------------------------------------------------------------------------------------------------ 1. rows
@pytest.mark.parametrize("name", CASES)
def test_rows_against_the_host_rows(name):
    basis, atoms = SR.case(name)
    B = SR.reference(name)
    got = _rows(basis, [atoms])
    err = np.abs(got - B).max()
    print(name, "F", basis.n_feats, "max |B|", np.abs(B).max(), "max error", err)
    assert err <= RTOL * np.abs(B).max()
    # the same call twice
    assert np.array_equal(got, _rows(basis, [atoms]))
    # ld > F: the padding is not written
    F = basis.n_feats
    padded = _rows(basis, [atoms], ld=F + 5, fill=np.nan)
    assert np.array_equal(padded[:, :F], got) and np.all(np.isnan(padded[:, F:]))


@pytest.mark.parametrize("name", ["unary", "mow", "uneven", "sym1", "pairs"])
def test_rows_against_site_energies_and_the_energy_row(name):
    basis, atoms = SR.case(name)
    atoms = wrapped(atoms)
    rows = _rows(basis, [atoms])
    model = ls.WeightedLinearModel(basis)
    c = np.random.default_rng(43).normal(0, 0.05, basis.n_feats)
    c[np.asarray(basis.col_idx, dtype=int)] = 0.0
    model.coefficients = c
    U = calculator.UFCalculator(model, md_skin=0.0).site_terms([atoms], virials=False)[0][0]
    assert np.abs(rows @ c - U).max() <= RTOL * np.abs(U).max(), np.abs(rows @ c - U).max()
    # (the featurizer leaves the frozen pair columns at zero: tests/test_site_rows_host.py)
    x_e = process.BasisFeaturizer(basis).featurize_frames([atoms], forces=False)[0][0]
    live = np.setdiff1d(np.arange(basis.n_feats), np.asarray(basis.col_idx, dtype=int))
    assert np.abs(rows.sum(0) - x_e)[live].max() <= RTOL * np.abs(x_e).max(), np.abs(rows.sum(0) - x_e)[live].max()


def test_rows_of_a_mixed_batch_do_not_depend_on_the_batch():
    basis, w16 = SR.case("unary")
    frames = [w16, _w1(), SR.case("cluster")[1], synthetic.lattice_frame("bcc", (2, 2, 3), 3.165, [74], seed=11), _sub(w16, 15)]
    together = _rows(basis, frames)
    off = np.concatenate([[0], np.cumsum([len(a) for a in frames])])
    for k, a in enumerate(frames):
        assert np.array_equal(together[off[k]:off[k + 1]], _rows(basis, [a])), k
    B = np.concatenate([SR.reference("unary"), SR.reference("cluster")])
    got = np.concatenate([together[off[0]:off[1]], together[off[2]:off[3]]])
    assert np.abs(got - B).max() <= RTOL * np.abs(B).max()
    ft = process.BasisFeaturizer(basis).site_rows(frames)
    assert np.array_equal(ft[0], together) and np.array_equal(ft[1], off)


# ------------------------------------------------------------------------------------------------ 2. fused grades
def _check_grades(basis, frames, w, label):
    B = _rows(basis, frames)
    g, fm, fa = _grades(basis, frames, w)
    want, bound = ls.leverage_reference(B, w, 1), ls.leverage_bound(B, w, 1)
    print(label, "max grade", want.max(), "worst error / bound", (np.abs(g - want) / bound).max())
    assert np.all(np.abs(g - want) <= bound), (label, (np.abs(g - want) / bound).max())
    off = np.concatenate([[0], np.cumsum([len(a) for a in frames])])
    for k in range(len(frames)):
        seg = g[off[k]:off[k + 1]]
        assert fm[k] == seg.max() and fa[k] == int(np.flatnonzero(seg == seg.max())[0]), (label, k)
    return B, g


@pytest.mark.parametrize("name", ["unary", "mow", "sym1", "cluster", "pairs"])
def test_fused_grades_within_the_derived_bound(name, report):
    basis, atoms = SR.case(name)
    _check_grades(basis, [atoms], _w(name), name)
    launches = report()
    assert launches and all(d["kernel"] == "k_site_grade" for d in launches), launches


def test_grades_on_the_far_side_of_the_switch(report):
    basis = _wide_basis()
    assert basis.n_feats > 608, basis.n_feats
    w = SR.seeded_model(basis).whitening()
    atoms = _w16()
    B, g = _check_grades(basis, [atoms, _sub(atoms, 5)], w, "wide")
    launches = report()
    assert launches and all(d["kernel"] == "k_site_rows+k_leverage" for d in launches), launches
    assert np.count_nonzero(B[:, int(sum(basis.get_feature_partition_sizes()[:2])):]) > 0      # 3-body columns in play
    assert np.array_equal(g, _grades(basis, [atoms, _sub(atoms, 5)], w)[0])


@pytest.mark.parametrize("n", [TILE - 1, TILE, TILE + 1])
def test_grades_at_the_tile_height(n, report):
    basis, _ = SR.case("unary")
    atoms = _sub(synthetic.lattice_frame("bcc", (2, 2, 3), 3.165, [74], seed=11), n)
    _, g = _check_grades(basis, [atoms], _w("unary"), f"n={n}")
    # ... and with a one-atom frame in the batch, in front: every tile boundary moves by one
    _, gb = _check_grades(basis, [_w1(), atoms, _w1()], _w("unary"), f"1+{n}+1")
    assert np.array_equal(gb[1:-1], g) and gb[0] == gb[-1]
    assert all(d["kernel"] == "k_site_grade" for d in report())


# ------------------------------------------------------------------------------------------------ 3. agreement, edge cases
@pytest.mark.parametrize("name", ["unary", "mow", "sym1"])
def test_fused_and_unfused_routes_agree(name):
    basis, atoms = SR.case(name)
    w = _w(name)
    model = SR.seeded_model(basis)
    B = _rows(basis, [atoms])
    unfused = model.site_leverage(B)                      # uf3_site_rows + uf3_leverage(group = 1)
    fused = _grades(basis, [atoms], w)[0]
    assert np.all(np.abs(fused - unfused) <= ls.leverage_bound(B, w, 1))
    assert np.array_equal(fused, _grades(basis, [atoms], w)[0])          # twice, bit for bit
    # frozen columns: W's zero rows and columns make a row's entries there irrelevant
    frozen = np.asarray(basis.col_idx, dtype=int)
    assert not w[frozen].any() and not w[:, frozen].any() and np.abs(B[:, frozen]).max() > 0
    B0 = B.copy()
    B0[:, frozen] = 0.0
    assert np.all(np.abs(fused - ls.leverage_reference(B0, w, 1)) <= ls.leverage_bound(B0, w, 1))
    # an all-zero W
    g0, fm0, fa0 = _grades(basis, [atoms], np.zeros_like(w))
    assert not g0.any() and not np.signbit(g0).any() and fm0[0] == 0.0 and fa0[0] == 0


def test_ties_go_to_the_lowest_index():
    basis, _ = SR.case("unary")
    w = _w("unary")
    perfect = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=1, rattle=0.0, strain=0.0)
    B = _rows(basis, [perfect])
    g, fm, fa = _grades(basis, [perfect, _w16()], w)
    gp = g[:16]
    bound = ls.leverage_bound(B, w, 1)
    assert np.all(np.abs(gp - gp[0]) <= bound + bound[0])              # symmetry-equivalent atoms
    assert fm[0] == gp.max() and fa[0] == int(np.flatnonzero(gp == gp.max())[0])
    assert fa[1] == int(np.argmax(g[16:])) and fm[1] == g[16:].max()


def test_an_empty_frame_gives_zero_and_minus_one():
    basis, w16 = SR.case("unary")
    w = np.ascontiguousarray(_w("unary"))
    ctx, db = _dev(basis)
    batch = _lib.FrameBatch([w16, SR.case("cluster")[1]])
    # the same atoms as three frames, the middle one empty (cell and pbc of the second given twice)
    off = np.array([0, 16, 16, 29], dtype=np.int64)
    cells = np.ascontiguousarray(np.concatenate([batch.cells[:1], batch.cells[1:2], batch.cells[1:2]]))
    pbc = np.ascontiguousarray(np.concatenate([batch.pbc[:1], batch.pbc[1:2], batch.pbc[1:2]]))
    fr = _lib.make_frames(off, cells, pbc)
    g, fm, fa = np.empty(29), np.full(3, np.nan), np.full(3, 7, dtype=np.int32)
    ctx.check(ctx.lib.uf3_site_grade(db.handle, C.byref(fr), _lib._p(batch.pos), _lib._p(batch.z), _lib._p(w), _lib._p(g), _lib._p(fm),
                                     _lib._p(fa)))
    ref = _grades(basis, [w16, SR.case("cluster")[1]], w)
    assert np.array_equal(g, ref[0])
    assert fm[1] == 0.0 and fa[1] == -1
    assert np.array_equal(fm[[0, 2]], ref[1]) and np.array_equal(fa[[0, 2]], ref[2])
    # the Python surface
    model = _graded_model()
    calc = calculator.UFCalculator(model, md_skin=0.0)
    empty = Atoms(numbers=[], positions=np.zeros((0, 3)), cell=np.eye(3) * 5.0, pbc=True)
    out = calc.get_site_grades([w16, empty, SR.case("cluster")[1]])
    assert list(out["offsets"]) == [0, 16, 16, 29] and out["frame_max"][1] == 0.0 and out["frame_argmax"][1] == -1
    wm = model.whitening()
    assert np.array_equal(out["grade"], _grades(basis, [w16, SR.case("cluster")[1]], wm)[0])
    one = calc.get_site_grades(w16)
    assert np.array_equal(one["grade"], out["grade"][:16]) and one["frame_max"] == out["frame_max"][0]
    assert one["frame_argmax"] == int(np.argmax(one["grade"]))
    # chunks under the atom limit: the same numbers
    chunked = calc.get_site_grades([w16, empty, SR.case("cluster")[1]], max_atoms_per_chunk=16)
    for k in ("grade", "frame_max", "frame_argmax"):
        assert np.array_equal(chunked[k], out[k]), k


# ------------------------------------------------------------------------------------------------ 4. meaning
def test_a_squeezed_atom_has_the_largest_grade():
    basis, _ = SR.case("unary")
    train = [wrapped(synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=100 + k)) for k in range(6)]
    fz = process.BasisFeaturizer(basis)
    x_e, x_f, off = fz.featurize_frames(train)
    x = np.concatenate([x_e / 16.0, x_f.reshape(-1, basis.n_feats)])
    model = ls.WeightedLinearModel(basis)
    mask = np.asarray(model.mask)
    y = np.random.default_rng(3).normal(0, 1, len(x))
    model.fit_with_gram(x[:, mask].T @ x[:, mask], x[:, mask].T @ y)
    w = model.whitening()
    g_train = _grades(basis, train, w)[0]
    pos = np.asarray(train[0].get_positions(), dtype=float).copy()
    cell = np.asarray(train[0].get_cell(), dtype=float)
    d = pos - pos[0]
    d -= np.round(d @ np.linalg.inv(cell)) @ cell
    r = np.linalg.norm(d, axis=1)
    r[0] = np.inf
    j = int(np.argmin(r))
    pos[0] = pos[0] + d[j] * 0.5               # to half the nearest-neighbour distance of its neighbour
    squeezed = Atoms(numbers=train[0].get_atomic_numbers(), positions=pos, cell=cell, pbc=True)
    g, fm, fa = _grades(basis, [squeezed], w)
    print("training max", g_train.max(), "squeezed frame", g)
    assert fa[0] == 0 and g[0] == g.max()
    assert g[0] > g_train.max()


# ------------------------------------------------------------------------------------------------ 5. / 6. MD
@functools.lru_cache(maxsize=None)
def _graded_model():
    """tests/golden/model_unary.json's coefficients with a seeded posterior on its basis"""
    model = ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json"))
    model.system_matrix, model._whitening = SR.seeded_model(model.bspline_config).system_matrix, None
    return model


def _md(friction=0.0, squeeze=False):
    calc = calculator.UFCalculator(_graded_model(), md_skin=0.0)
    frames = [_w16(), synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=13)]
    if squeeze:         # one atom a quarter of the way towards its nearest neighbour: the grades move while it is pushed back
        pos = np.asarray(frames[1].get_positions(), dtype=float).copy()
        cell = np.asarray(frames[1].get_cell(), dtype=float)
        d = pos - pos[3]
        d -= np.round(d @ np.linalg.inv(cell)) @ cell
        r = np.linalg.norm(d, axis=1)
        r[3] = np.inf
        pos[3] += 0.25 * d[int(np.argmin(r))]
        frames[1] = Atoms(numbers=frames[1].get_atomic_numbers(), positions=pos, cell=cell, pbc=True)
    dyn = MolecularDynamics(calc, frames, 1.0, masses={"W": 183.84}, temperature_K=600.0, friction_per_fs=friction, seed=7)
    dyn.initialize_velocities(600.0, seed=3)
    return calc, dyn


def _same_state(a, b):
    return np.array_equal(a.get_positions(), b.get_positions()) and np.array_equal(a.get_velocities(), b.get_velocities()) \
        and a.step == b.step


@pytest.mark.parametrize("friction", [0.0, 0.02], ids=["nve", "langevin"])
def test_md_samples_leave_the_trajectory_alone(friction):
    calc, dyn = _md(friction)
    rec = dyn.run(6, thermo_every=3, grade_every=2)
    assert rec["grade"].shape == (3, 2) and rec["grade_atom"].shape == (3, 2) and rec["grade_atom"].dtype == np.int64
    assert list(rec["grade_step"]) == [2, 4, 6] and rec["steps_done"] == 6
    _, plain = _md(friction)
    ref = plain.run(6, thermo_every=3)
    assert _same_state(dyn, plain)
    for k in ref:
        assert np.array_equal(rec[k], ref[k]), k
    # each record is get_site_grades of the state run(s k) stops in
    _, twin = _md(friction)
    basis = calc.model.bspline_config
    w = calc.model.whitening()
    for s in range(3):
        twin.run(2)
        atoms = twin.get_atoms()
        want = calc.get_site_grades(atoms)
        bound = ls.leverage_bound(_rows(basis, atoms), w, 1)
        off = want["offsets"]
        for f in range(2):
            seg, b = want["grade"][off[f]:off[f + 1]], bound[off[f]:off[f + 1]]
            assert abs(rec["grade"][s, f] - want["frame_max"][f]) <= b.max(), (s, f)
            # the atom named holds the maximum within the bound
            assert seg[rec["grade_atom"][s, f]] >= seg.max() - 2 * b.max(), (s, f)
    # run(4); run(2) = run(6)
    _, split = _md(friction)
    a, b = split.run(4, thermo_every=3, grade_every=2), split.run(2, thermo_every=3, grade_every=2)
    assert _same_state(split, dyn)
    for k in ("grade", "grade_atom", "grade_step"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), rec[k]), k
    assert a["steps_done"] == 4 and b["steps_done"] == 2


def test_md_stops_at_the_threshold():
    k, n = 5, 60
    # a free run whose maxima rise somewhere: the thermal one, else the one that starts with a displaced atom
    for squeeze in (False, True):
        _, free = _md(squeeze=squeeze)
        maxima = free.run(n, grade_every=k)["grade"].max(axis=1)
        print("squeeze", squeeze, "maxima of the free run", maxima)
        rising = [s for s in range(1, len(maxima)) if maxima[s] > maxima[:s].max()]
        if rising:
            break
    assert rising, "no sample exceeds every earlier one: choose another start"
    s = rising[0]
    stop = 0.5 * (maxima[s] + maxima[:s].max())
    _, dyn = _md(squeeze=squeeze)
    rec = dyn.run(n, thermo_every=1, grade_every=k, grade_stop=stop)
    done = (s + 1) * k
    assert rec["steps_done"] == done and dyn.step == done
    assert rec["grade"].shape == (s + 1, 2) and np.array_equal(rec["grade"].max(axis=1), maxima[:s + 1])
    assert len(rec["step"]) == done and list(rec["grade_step"]) == list(range(k, done + 1, k))
    _, twin = _md(squeeze=squeeze)
    ref = twin.run(done, thermo_every=1)
    assert _same_state(dyn, twin)
    for key in ref:
        assert np.array_equal(rec[key], ref[key]), key
    # a following run goes on as run(n) would have
    tail = dyn.run(n - done, thermo_every=1)
    _, whole = _md(squeeze=squeeze)
    all_ = whole.run(n, thermo_every=1)
    assert _same_state(dyn, whole)
    for key in all_:
        assert np.array_equal(np.concatenate([rec[key], tail[key]]), all_[key]), key
    # a threshold that is never exceeded, and none
    _, calm = _md(squeeze=squeeze)
    assert calm.run(n, grade_every=k, grade_stop=2.0 * maxima.max())["steps_done"] == n
    assert np.array_equal(calm.get_positions(), free.get_positions())


# ------------------------------------------------------------------------------------------------ 7. errors
def test_error_codes():
    basis, w16 = SR.case("unary")
    ctx, db = _dev(basis)
    batch = _lib.FrameBatch([w16])
    F = db.n_feat
    w = np.ascontiguousarray(_w("unary"))
    g = np.empty(16)
    args = (db.handle, C.byref(batch.struct), _lib._p(batch.pos), _lib._p(batch.z))
    assert ctx.lib.uf3_site_grade(*args, None, _lib._p(g), None, None) == 1                       # a null W
    assert ctx.lib.uf3_site_rows(*args, _lib._p(np.empty((16, F))), F - 1) == 1                  # ld < F
    assert ctx.lib.uf3_site_rows(*args, None, F) == 1
    alien = Atoms(numbers=[74, 42], positions=[[0, 0, 0], [1.5, 1.5, 1.5]], cell=np.eye(3) * 6.0, pbc=True)
    ab = _lib.FrameBatch([alien])
    assert ctx.lib.uf3_site_grade(db.handle, C.byref(ab.struct), _lib._p(ab.pos), _lib._p(ab.z), _lib._p(w), _lib._p(np.empty(2)),
                                  None, None) == 2                                                # UF3_ESPECIES
    assert ctx.lib.uf3_site_rows(db.handle, C.byref(ab.struct), _lib._p(ab.pos), _lib._p(ab.z), _lib._p(np.empty((2, F))), F) == 2
    # W of the wrong size, at the Python layer
    other = SR.seeded_model(SR.case("pairs")[0])
    with pytest.raises(ValueError, match="basis"):
        from uf3_amd import pipeline
        pipeline.DeviceLeverage(other, process.BasisFeaturizer(basis))
    # the MD entry: a grades buffer with no sample due and the reverse, as for thermo and flux
    calc, dyn = _md()
    h, lib = dyn._live(), ctx.lib
    d_w = dyn._grade_w(calc.model.whitening())
    done = C.c_int64(-1)
    buf = np.zeros((4, 2, 2))
    run = lambda n, every, grades, dw=d_w: lib.uf3_md_run_grade(h, n, 1.0, 0.0, 0.0, 0, 0.5, 0, 0, None, dw, every, 0.0, grades,  # noqa: E731
                                                                C.byref(done))
    assert run(4, 0, _lib._p(buf)) == 1 and run(1, 2, _lib._p(buf)) == 1
    assert run(4, 2, None) == 1
    assert run(4, -1, None) == 1
    assert run(4, 2, _lib._p(buf), None) == 1                                                     # a null W with samples due
    assert dyn.step == 0 and done.value == 0
    assert run(4, 2, _lib._p(buf)) == 0 and done.value == 4 and dyn.step == 4
    with pytest.raises(_lib.UF3Error):
        dyn.run(4, grade_every=2, flux_every=2)
