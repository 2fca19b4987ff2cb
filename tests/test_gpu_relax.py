"""Batched relaxation on the device (``uf3_relax_*``, ``uf3_amd.forcefield.relax``) against the NumPy restatement in
tests/_relax_ref.py, whose forces come from ``UFCalculator.evaluate_frames``: step-by-step parity with and without the cell on
3-body and 2-body models, converged frames that are converged, the bcc W lattice constant, batch independence, cadence and
split invariance, edge cases, and the context left as it was found."""
import os

import numpy as np
import pytest

from uf3_amd import _lib, synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator
from uf3_amd.forcefield.relax import Relaxation
from uf3_amd.regression import least_squares as ls
import _relax_ref as R
from _util import GOLDEN, load_case

pytestmark = pytest.mark.gpu
A0_W = 3.17352          # model_unary.json: zero virial trace (the value tests/test_gpu_harmonic.py pins)
TOL = 1e-9


def _unary():
    return calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json")), md_skin=0.0)


def _mow():
    basis = synthetic.notebook_basis(["Mo", "W"])
    model = ls.WeightedLinearModel(basis)
    coeff = np.random.default_rng(31).normal(0, 0.05, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    model.coefficients = coeff
    return calculator.UFCalculator(model, md_skin=0.0)


def _binary():
    return calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_binary.json")), md_skin=0.0)


def _vacancy(seed, reps=(4, 4, 4), rattle=0.05):
    a = synthetic.lattice_frame("bcc", reps, A0_W, [74], seed=seed, rattle=rattle, strain=0.0)
    return Atoms(numbers=a.get_atomic_numbers()[1:], positions=a.get_positions()[1:], cell=a.get_cell(), pbc=True)


def _cluster():
    a = synthetic.lattice_frame("bcc", (2, 2, 2), A0_W, [74], seed=5, rattle=0.05, strain=0.0)
    return Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions(), cell=np.zeros((3, 3)), pbc=False)


def _mow54():
    return synthetic.lattice_frame("bcc", (3, 3, 3), 3.2, [42, 74], seed=84, rattle=0.05)


def _slab():
    a = synthetic.lattice_frame("bcc", (3, 3, 2), 3.2, [42, 74], seed=9, rattle=0.05)
    return Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions(), cell=a.get_cell(), pbc=[True, True, False])


def _w300():
    # 300 atoms: two chunks of the drivers' chunk table (256 + 44), the second partly filled
    return synthetic.lattice_frame("bcc", (5, 5, 6), A0_W, [74], seed=11, rattle=0.05, strain=0.0)


def _batches():
    return {"w_vacancy_cluster": (_unary, lambda: [_vacancy(3), _cluster()]),
            "w300_two_chunks": (_unary, lambda: [_cluster(), _w300(), _vacancy(8, reps=(3, 3, 3))]),
            "mow54_slab": (_mow, lambda: [_mow54(), _slab()]),
            "nexe_2body": (_binary, lambda: [load_case("case_nexe32")[2]])}


def _reference(calc, frames, relax_cell=False, fixed=None):
    off = np.cumsum([0] + [len(a) for a in frames])

    def evaluate(x, cells):
        moved = [Atoms(numbers=a.get_atomic_numbers(), positions=x[off[k]:off[k + 1]], cell=cells[k], pbc=a.get_pbc())
                 for k, a in enumerate(frames)]
        e, f, _, w = calc.evaluate_frames(moved, virial=True)
        return e, f, w
    x0 = np.concatenate([a.get_positions() for a in frames])
    return R.Fire(evaluate, x0, [np.array(a.get_cell(), dtype=float) for a in frames], [a.get_pbc() for a in frames], off,
                  relax_cell=relax_cell, fixed=fixed)


STATUS = {R.RUNNING: "running", R.CONVERGED: "converged", R.NONFINITE: "nonfinite"}


@pytest.mark.parametrize("relax_cell", [False, True], ids=["positions", "cell"])
@pytest.mark.parametrize("name", ["w_vacancy_cluster", "w300_two_chunks", "mow54_slab", "nexe_2body"])
def test_parity_with_the_restatement(name, relax_cell):
    make_calc, make_frames = _batches()[name]
    calc, frames = make_calc(), make_frames()
    ref = _reference(calc, frames, relax_cell)
    fmax, kw = 1e-3, dict(dt=0.1, dt_max=1.0, maxstep=0.2)
    with Relaxation(calc, frames, relax_cell=relax_cell) as rel:
        for k in range(30):
            out = rel.run(1, fmax=fmax, **kw)
            ref.run(1, fmax=fmax, **kw)
            x = rel.get_positions()
            assert np.abs(x - ref.x).max() <= TOL, (k, np.abs(x - ref.x).max())
            assert np.abs(out["energy"] - ref.e_last).max() <= TOL, (k, out["energy"], ref.e_last)
            assert np.abs(rel.get_cells() - ref.cells).max() <= TOL
        out = rel.run(400, fmax=fmax, **kw)
        ref.run(400, fmax=fmax, **kw)
        assert out["status"] == [STATUS[s] for s in ref.status]
        assert out["steps"].tolist() == ref.steps.tolist()
        assert np.abs(rel.get_positions() - ref.x).max() <= 1e-7
        if relax_cell:
            assert np.abs(rel.get_cells() - ref.cells).max() <= 1e-7
            per = [bool(np.all(a.get_pbc())) for a in frames]
            for k in range(len(frames)):
                assert per[k] or np.array_equal(rel.get_cells()[k], np.asarray(frames[k].get_cell(), dtype=float))
        else:
            assert np.array_equal(rel.get_cells(), np.array([a.get_cell() for a in frames], dtype=float))


@pytest.mark.parametrize("relax_cell", [False, True], ids=["positions", "cell"])
def test_converged_frames_are_converged(relax_cell):
    calc = _unary()
    frames = [_vacancy(3), _cluster(), _vacancy(4)]
    e0 = calc.evaluate_frames(frames)[0]
    fmax = 1e-3
    relaxed, info = calc.relax_frames(frames, fmax=fmax, relax_cell=relax_cell, max_steps=1000)
    assert np.all(info["converged"]) and info["status"] == ["converged"] * 3
    e, f, off, w = calc.evaluate_frames(relaxed, virial=True)
    assert np.sqrt((f * f).sum(1)).max() < fmax
    assert np.all(e < e0)
    assert np.abs(e - info["energy"]).max() <= 1e-9
    for k, a in enumerate(relaxed):
        if relax_cell and np.all(a.get_pbc()):
            D = np.linalg.inv(np.asarray(frames[k].get_cell(), dtype=float)) @ np.asarray(a.get_cell(), dtype=float)
            G = R.cell_force(D, R.voigt_to_matrix(w[k]), len(a))
            assert np.sqrt((G * G).sum(1)).max() < fmax
    with pytest.warns(RuntimeWarning, match="did not converge"):
        calc.relax_frames(frames, fmax=fmax, max_steps=3)


def test_bcc_w_lattice_constant_under_cell_relaxation():
    calc = _unary()
    base = np.array([[0, 0, 0], [0.5, 0.5, 0.5]])
    grid = np.array(list(np.ndindex(4, 4, 4)), dtype=float)
    frac = ((grid[:, None, :] + base[None]) / 4).reshape(-1, 3)
    strain = 0.02 * np.eye(3)
    strain[0, 1] = strain[1, 0] = 0.01
    cell = np.diag([4 * A0_W] * 3) @ (np.eye(3) + strain)
    atoms = Atoms(numbers=np.full(128, 74), positions=frac @ cell, cell=cell, pbc=True)
    (relaxed,), info = calc.relax_frames([atoms], fmax=1e-4, relax_cell=True, max_steps=3000)
    assert info["converged"][0]
    c = np.asarray(relaxed.get_cell(), dtype=float)
    assert np.abs(np.linalg.norm(c, axis=1) / 4 - A0_W).max() <= 1e-4, c
    assert np.abs(c - np.diag(np.diag(c))).max() < 1e-4, c


def test_frames_relax_alike_alone_and_in_a_batch():
    calc = _unary()
    frames = [_vacancy(3), _cluster(), _vacancy(7), _vacancy(8, reps=(3, 3, 3))]
    with Relaxation(calc, frames) as rel:
        batch = rel.run(600, fmax=1e-3)
        xb = rel.get_positions()
    off = np.cumsum([0] + [len(a) for a in frames])
    for k, a in enumerate(frames):
        with Relaxation(calc, [a]) as rel:
            alone = rel.run(600, fmax=1e-3)
            x = rel.get_positions()
        assert alone["status"][0] == batch["status"][k] and alone["steps"][0] == batch["steps"][k]
        assert np.abs(x - xb[off[k]:off[k + 1]]).max() <= 1e-8


@pytest.mark.parametrize("relax_cell", [False, True], ids=["positions", "cell"])
def test_cadence_and_splitting_do_not_change_the_result(relax_cell):
    calc = _unary()
    frames = [_vacancy(3), _cluster(), _vacancy(9)]
    finals = []
    for every in (1, 50):
        with Relaxation(calc, frames, relax_cell=relax_cell) as rel:
            out = rel.run(500, fmax=1e-3, check_every=every)
            finals.append((rel.get_positions(), rel.get_cells(), out["status"], out["steps"], out["energy"]))
    (x1, c1, s1, n1, e1), (x2, c2, s2, n2, e2) = finals
    assert np.array_equal(x1, x2) and np.array_equal(c1, c2) and s1 == s2 and np.array_equal(n1, n2) and np.array_equal(e1, e2)
    with Relaxation(calc, frames, relax_cell=relax_cell) as rel:
        rel.run(37, fmax=1e-3)
        out = rel.run(463, fmax=1e-3)
        assert out["status"] == s1 and np.array_equal(out["steps"], n1)
        assert np.abs(rel.get_positions() - x1).max() <= 1e-10
        assert np.abs(rel.get_cells() - c1).max() <= 1e-10


def test_records_follow_the_run():
    calc = _unary()
    frames = [_vacancy(3), _cluster()]
    with Relaxation(calc, frames) as rel:
        out = rel.run(400, fmax=1e-3, record_every=5)
    rec = out["records"]
    assert rec["energy"].shape == (81, 2) and rec["iteration"][:3].tolist() == [0, 5, 10]
    assert np.abs(rec["energy"][-1] - out["energy"]).max() <= TOL and np.array_equal(rec["fmax"][-1], out["fmax"])
    assert np.all(rec["energy"][0] > rec["energy"][-1])


def test_edge_cases():
    calc = _unary()
    # a frame that starts converged takes no step and comes back bit for bit
    done = _vacancy(3)
    (relaxed,), _ = calc.relax_frames([done], fmax=1e-3, max_steps=1000)
    with Relaxation(calc, [relaxed, _vacancy(5)]) as rel:
        out = rel.run(500, fmax=1e-2)
        assert out["steps"][0] == 0 and out["status"][0] == "converged" and out["steps"][1] > 0
        assert np.array_equal(rel.get_positions()[:len(relaxed)], np.asarray(relaxed.get_positions()))
        assert np.array_equal(rel.get_cells()[0], np.asarray(relaxed.get_cell(), dtype=float))
    # fixed atoms do not move
    frames = [_vacancy(3), _cluster()]
    n = sum(len(a) for a in frames)
    fixed = np.zeros(n, bool)
    fixed[[0, 5, 130]] = True
    x0 = np.concatenate([a.get_positions() for a in frames])
    with Relaxation(calc, frames, fixed=fixed) as rel:
        out = rel.run(600, fmax=1e-3)
        x = rel.get_positions()
    assert np.all(out["converged"])
    assert np.array_equal(x[fixed], x0[fixed]) and not np.allclose(x[~fixed], x0[~fixed])
    ref = _reference(calc, frames, fixed=fixed)
    ref.run(600, fmax=1e-3)
    assert ref.steps.tolist() == out["steps"].tolist() and np.abs(ref.x - x).max() <= 1e-7
    # running out of steps: not converged, steps == max_steps
    with Relaxation(calc, [_vacancy(3)]) as rel:
        out = rel.run(7, fmax=1e-6)
    assert not out["converged"][0] and out["status"] == ["running"] and out["steps"].tolist() == [7]


def test_library_refuses_bad_arguments():
    calc = _unary()
    with Relaxation(calc, [_vacancy(3)]) as rel:
        lib, h = rel.ctx.lib, rel.handle
        buf = np.zeros((3, 1, 2))
        assert lib.uf3_relax_run(h, 10, 1e-3, 0.1, 1.0, 0.2, 0.5, 1, 5, None) == 1
        assert lib.uf3_relax_run(h, 10, 1e-3, 0.1, 1.0, 0.2, 0.5, 1, 0, _lib._p(buf)) == 1
        assert lib.uf3_relax_run(h, 10, 0.0, 0.1, 1.0, 0.2, 0.5, 1, 0, None) == 1
        assert lib.uf3_relax_run(h, 10, 1e-3, 0.1, 1.0, 0.2, 0.5, 0, 0, None) == 1
        assert lib.uf3_relax_run(h, -1, 1e-3, 0.1, 1.0, 0.2, 0.5, 1, 0, None) == 1
        assert lib.uf3_relax_run(h, 10, 1e-3, 0.1, 1.0, 0.2, 5.0, 1, 0, None) == 1


def test_runs_leave_the_context_and_the_calculator_as_they_were():
    calc = _unary()
    ctx = _lib.get_context(calc.device)
    other = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=61)
    e0, f0, _ = calc.evaluate_frames([other])                    # (md_skin 0: the context's skin is 0)
    steps0 = ctx.md_stats()["steps"]
    with Relaxation(calc, [_vacancy(3)], skin=0.7) as rel:
        rel.run(20, fmax=1e-3)
    with Relaxation(calc, [_vacancy(3)], relax_cell=True) as rel:
        rel.run(5, fmax=1e-3)
    foreign = _vacancy(4)
    foreign.numbers[:3] = 42                                      # Mo: outside the unary basis
    rel = Relaxation(calc, [foreign])
    with pytest.raises(_lib.SpeciesError):
        rel.run(3)
    rel.close()
    steps1 = ctx.md_stats()["steps"]
    e1, f1, _ = calc.evaluate_frames([other])
    e2, f2, _ = calc.evaluate_frames([other])
    assert ctx.md_stats()["steps"] == steps1 and getattr(ctx, "_md_skin", 0.0) == 0.0
    assert steps1 > steps0
    assert np.array_equal(e0, e1) and np.array_equal(f0, f1) and np.array_equal(e1, e2)
