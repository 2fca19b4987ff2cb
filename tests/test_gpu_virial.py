"""
The evaluator's strain derivative dE/d(strain) (``uf3_eval_virial[_dev]``, ``uf3_eval_atoms``, ``uf3_eval_centres``; Voigt xx, yy,
zz, yz, xz, xy, eV) against the oracle's (``uf3o_eval_virial``, pinned to finite differences of its own energy in
tests/test_oracle_virial.py) on every route and kernel instance, frame by frame and step by step, with energies and forces
alongside.  Every test runs on a fresh context made with UF3_DEBUG_LDS set, whose evaluator names on stderr the k_eval instance
each call launched: the tests assert that the route they mean to reach is the one that ran.
"""
import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic, _lib
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator
from uf3_amd.regression import least_squares as ls
from _util import dbg, worst_elementwise  # noqa: F401  (dbg: the fixture)

pytestmark = pytest.mark.gpu
TOL = 1e-9                  # energies (relative) and forces (entry by entry), as in tests/test_gpu_parity.py
MOW, NUMS = ['Mo', 'W'], [42, 74]


def _model(basis, seed):
    model = ls.WeightedLinearModel(basis)
    coeff = np.random.default_rng(seed).normal(0, 0.05, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    model.coefficients = coeff
    return model, coeff


def _check_frame(e, f, v, ob, atoms, coeff, label="", ref=None):
    e_o, f_o, v_o = ref if ref is not None else O.evaluate(ob, atoms, coeff, virial=True)
    assert abs(e - e_o) <= TOL * max(1.0, abs(e_o)), (label, e, e_o)
    if f is not None:
        assert worst_elementwise(f, f_o, TOL) <= 1.0, label
    assert worst_elementwise(v, v_o, rtol=1e-9, floor=1e-11) <= 1.0, (label, v, v_o)
    return v_o


def _check_batch(out, ob, frames, coeff, label=""):
    e, f, off, v = out
    assert v.shape == (len(frames), 6) and np.all(np.isfinite(v))
    for k, atoms in enumerate(frames):
        _check_frame(e[k], None if f is None else f[off[k]:off[k + 1]], v[k], ob, atoms, coeff, f"{label} frame {k}")


def _frame(a, pbc=None, positions=None, cell=None):
    return Atoms(numbers=a.get_atomic_numbers(), positions=a.get_positions() if positions is None else positions,
                 cell=a.get_cell() if cell is None else cell, pbc=a.get_pbc() if pbc is None else pbc)


def _primitive():
    cell = np.array([[2.9, 0.0, 0.0], [0.7, 2.8, 0.0], [0.4, -0.6, 3.1]])
    return Atoms(numbers=[42, 74], positions=np.array([[0.03, 0.02, 0.01], [0.52, 0.47, 0.55]]) @ cell, cell=cell, pbc=True)


def _small_frames():
    """the Mo/W frames of tests/test_oracle_virial.py and of the MD route's small-cell test"""
    tiny = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, NUMS, seed=81)
    a = synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, NUMS, seed=84)
    shear = np.eye(3) + np.array([[0, 0.18, 0.07], [0, 0, -0.12], [0, 0, 0]])
    triclinic = _frame(a, positions=a.get_positions() @ shear, cell=np.asarray(a.get_cell()) @ shear)
    slab = _frame(synthetic.lattice_frame("bcc", (4, 4, 3), 3.165, NUMS, seed=82), pbc=[True, True, False])
    cluster = _frame(synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, NUMS, seed=83), pbc=False)
    return {"primitive": _primitive(), "tiny_cell": tiny, "triclinic": triclinic, "slab": slab, "cluster": cluster,
            "bcc_433": synthetic.lattice_frame("bcc", (4, 3, 3), 3.165, NUMS, seed=87)}


def test_plain_route_on_a_ragged_batch_host_and_device_entries(dbg):
    """md_skin = 0: one ragged batch of tiny, skewed, slab and cluster frames (per-frame strain rows, frame offsets), with forces
    (the centre pass + collection pass), without forces (what _get_stress calls: the gather instance), and through
    uf3_eval_virial_dev with every input and output in device memory."""
    import ctypes as C
    import torch
    basis = dbg.basis(synthetic.notebook_basis(MOW))
    model, coeff = _model(basis, 31)
    ob = O.OracleBasis(basis)
    calc = calculator.UFCalculator(model, md_skin=0.0)
    frames = list(_small_frames().values())
    for _ in range(2):
        calc.evaluate_frames(frames, virial=True)                   # (list capacity tuned)
    dbg.launches()
    out = calc.evaluate_frames(frames, virial=True)
    said = dbg.launches()
    assert said and all(s["vir"] == 1 and s["md"] == 0 and s["gather"] == 0 for s in said), said
    _check_batch(out, ob, frames, coeff, "plain")
    e_only = calc.evaluate_frames(frames, forces=False, virial=True)
    said = dbg.launches()
    assert said and all(s["vir"] == 1 and s["gather"] == 1 for s in said), said
    assert e_only[1] is None
    _check_batch(e_only, ob, frames, coeff, "forces=False")
    # device-resident entry
    ctx = _lib.get_context(None)
    db = _lib.device_basis(basis, ctx)
    batch = _lib.FrameBatch(frames)
    dev = torch.device("cuda", ctx.device)
    d_pos, d_z = torch.from_numpy(batch.pos).to(dev), torch.from_numpy(batch.z).to(dev)
    d_e = torch.zeros(batch.n_frames, dtype=torch.float64, device=dev)
    d_f = torch.zeros((batch.n_atoms, 3), dtype=torch.float64, device=dev)
    d_v = torch.full((batch.n_frames, 6), np.nan, dtype=torch.float64, device=dev)
    prev = ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    try:
        ctx.check(ctx.lib.uf3_eval_virial_dev(db.handle, C.byref(batch.struct), C.c_void_p(d_pos.data_ptr()),
                                              C.c_void_p(d_z.data_ptr()), *calc._pc, C.c_void_p(d_e.data_ptr()),
                                              C.c_void_p(d_f.data_ptr()), C.c_void_p(d_v.data_ptr())))
        ctx.synchronize()
    finally:
        ctx.restore_stream(prev)
    said = dbg.launches()
    assert said and all(s["vir"] == 1 for s in said), said
    _check_batch((d_e.cpu().numpy(), d_f.cpu().numpy(), batch.offsets, d_v.cpu().numpy()), ob, frames, coeff, "_dev")


# (switch, what the debug line must say on every step of the walk; None: not asserted)
_MD_ROUTES = {
    "default": ({}, {"md": 1, "gather": 0}),
    "no_cw": ({"UF3_EVAL_NO_CW": "1"}, {"md": 1, "cw": 0, "win": 0, "tab": 1}),     # (the switch turns WIN off too)
    "no_tab": ({"UF3_EVAL_NO_TAB": "1"}, {"md": 1, "cw": 0, "win": 0, "tab": 0}),
    "no_cap16": ({"UF3_EVAL_NO_CAP16": "1"}, {"md": 1, "cap16": 0}),
    "gather": ({"UF3_EVAL_GATHER": "1"}, {"md": 0, "gather": 1}),
    "separate_n3": ({"UF3_SEPARATE_N3": "1"}, {"md": 0, "gather": 0}),
    "no_md": ({"UF3_NO_MD": "1"}, {"md": 0, "gather": 0}),
}


@pytest.mark.parametrize("density", ["short_lists", "long_lists"])
@pytest.mark.parametrize("route", list(_MD_ROUTES))
def test_md_route_instances_on_every_step_of_a_walk(route, density, dbg, monkeypatch):
    """The MD skin route (persistent lists, skin 0.5) and every switch that takes a step elsewhere, on bcc Mo/W with 3-body lists
    of at most 16 entries (the CW instances by default, the WIN instances without them) and on a compressed cell whose lists hold
    26 (the one-wave instances): energy, forces and strain derivative against the oracle on every step."""
    env, want = _MD_ROUTES[route]
    basis = dbg.basis(synthetic.notebook_basis(MOW))
    model, coeff = _model(basis, 41)
    ob = O.OracleBasis(basis)
    if density == "short_lists":
        start = synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, NUMS, seed=51)
    else:
        start = synthetic.lattice_frame("bcc", (4, 4, 4), 2.4, NUMS, seed=52, rattle=0.03, strain=0.0)
    plain = calculator.UFCalculator(model, md_skin=0.0)
    for _ in range(2):
        plain.evaluate_frames([start], virial=True)                  # (capacity tuned: the MD route starts from a tuned context)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    calc = calculator.UFCalculator(model, md_skin=0.5)
    rng = np.random.default_rng(6)
    pos = start.get_positions()
    dbg.launches()
    for step in range(6):
        pos = pos + rng.uniform(-0.03, 0.03, pos.shape)
        atoms = _frame(start, positions=pos)
        out = calc.evaluate_frames([atoms], virial=True)
        said = dbg.launches()
        assert said and said[-1]["vir"] == 1, said
        for key, val in want.items():
            assert said[-1][key] == val, (route, density, step, said)
        if density == "long_lists":
            assert said[-1]["cap"] > 16 and said[-1]["cw"] == 0, said
            if route == "default":
                assert said[-1]["win"] == 1, said                              # (the window table read from global memory)
        elif route in ("default", "no_cap16"):
            assert said[-1]["cw"] == 1 and said[-1]["cap"] <= 16, said           # (the CW instances: both cap16 settings)
        _check_batch(out, ob, [atoms], coeff, f"{route} {density} step {step}")


@pytest.mark.parametrize("case", ["tiny_cell", "slab", "cluster", "triclinic", "ragged_batch"])
def test_md_route_on_small_cells_slabs_clusters_and_batches(case, dbg):
    """The MD route where lists hold several images of one neighbour, with open boundaries, on a skewed cell and on a ragged
    batch: the strain derivative of every step against the oracle."""
    basis = dbg.basis(synthetic.notebook_basis(MOW))
    model, coeff = _model(basis, 24)
    ob = O.OracleBasis(basis)
    small = _small_frames()
    frames = ([small["bcc_433"], small["tiny_cell"], small["primitive"], small["triclinic"]] if case == "ragged_batch"
              else [small[case]])
    plain = calculator.UFCalculator(model, md_skin=0.0)
    for _ in range(2):
        plain.evaluate_frames(frames)
    calc = calculator.UFCalculator(model, md_skin=0.4)
    rng = np.random.default_rng(12)
    dbg.launches()
    for step in range(6):
        frames = [_frame(f, positions=f.get_positions() + rng.uniform(-0.03, 0.03, (len(f), 3))) for f in frames]
        out = calc.evaluate_frames(frames, virial=True)
        said = dbg.launches()
        assert said and said[-1]["md"] == 1 and said[-1]["vir"] == 1, said
        _check_batch(out, ob, frames, coeff, f"{case} step {step}")


@pytest.mark.parametrize("bar_off", [False, True])
def test_small_md_steps_through_the_bar_staged_block(bar_off, dbg, monkeypatch):
    """128-atom MD steps: positions stored through the BAR into device memory (the default on a large-BAR device) or fetched
    from the pinned block (UF3_NO_BAR_STAGE, read when the context is made): the strain derivative of every step."""
    if bar_off:
        monkeypatch.setenv("UF3_NO_BAR_STAGE", "1")
    basis = dbg.basis(synthetic.notebook_basis(MOW))
    model, coeff = _model(basis, 4)
    ob = O.OracleBasis(basis)
    start = synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, NUMS, seed=8)
    calc = calculator.UFCalculator(model, md_skin=0.4)
    rng = np.random.default_rng(2)
    pos = start.get_positions()
    for step in range(10):
        pos = pos + rng.uniform(-0.02, 0.02, pos.shape)
        if step == 6:
            pos[5] += [0.3, 0.1, -0.2]                                # (outruns the lists: the step repeats itself)
        atoms = _frame(start, positions=pos)
        out = calc.evaluate_frames([atoms], virial=True)
        _check_batch(out, ob, [atoms], coeff, f"bar_off={bar_off} step {step}")
    said = dbg.launches()
    assert sum(s["md"] for s in said) >= 9, said
    st = _lib.get_context(None).md_stats()
    assert st["steps"] >= 10 and st["redone"] >= 1, st


@pytest.mark.parametrize("part_sums", [True, False])
def test_collection_pass_sums_of_a_large_frame(part_sums, dbg, monkeypatch):
    """One whole frame of >= 8192 atoms on the MD route: the per-workgroup sums of the collection pass (and UF3_NO_PART_SUMS, the
    per-atom sums) against the oracle on moved steps."""
    if not part_sums:
        monkeypatch.setenv("UF3_NO_PART_SUMS", "1")
    atoms, basis = synthetic.config_c4(frame=2)
    dbg.basis(basis)
    model, coeff = _model(basis, 8)
    ob = O.OracleBasis(basis)
    calc = calculator.UFCalculator(model, md_skin=0.5)
    a = atoms.copy()
    dbg.launches()
    for step in range(3):
        a.positions = a.positions + np.random.default_rng(40 + step).uniform(-0.02, 0.02, a.positions.shape)
        out = calc.evaluate_frames([a], virial=True)
        said = dbg.launches()
        assert said and said[-1]["atoms"] >= 8192, said
        if step > 0:                                                 # (a fresh context's first call tunes the lists: plain route)
            assert said[-1]["md"] == 1 and said[-1]["part_sums"] == int(part_sums), said
        _check_batch(out, ob, [a], coeff, f"part_sums={part_sums} step {step}")


def test_fifty_thousand_atom_ternary(dbg):
    """configs[4]: the 50 000-atom V/Mo/W cell through the plain route and the MD route's first steps."""
    atoms, basis = synthetic.config_c5()
    dbg.basis(basis)
    model, coeff = _model(basis, 11)
    ob = O.OracleBasis(basis)
    ref = O.evaluate(ob, atoms, coeff, virial=True)
    e, f, _, v = calculator.UFCalculator(model, md_skin=0.0).evaluate_frames([atoms], virial=True)
    _check_frame(e[0], f, v[0], ob, atoms, coeff, "plain", ref)
    md = calculator.UFCalculator(model, md_skin=0.5)
    md.evaluate_frames([atoms], virial=True)
    e, f, _, v = md.evaluate_frames([atoms], virial=True)
    said = dbg.launches()
    assert said[-1]["md"] == 1 and said[-1]["part_sums"] == 1, said
    _check_frame(e[0], f, v[0], ob, atoms, coeff, "md", ref)


def test_atom_and_centre_shares_and_the_sharded_drivers(dbg, monkeypatch):
    """uf3_eval_atoms (the gather route on a block) and uf3_eval_centres (the centre pass on a block + its halo) at world sizes
    3 and 8, summed; a block of centres with UF3_NO_HALO; parallel.sharded_evaluate and ShardedEvaluator on one GPU."""
    import torch
    from uf3_amd import parallel
    basis = dbg.basis(synthetic.notebook_basis(MOW))
    model, coeff = _model(basis, 5)
    ob = O.OracleBasis(basis)
    atoms = synthetic.lattice_frame("bcc", (5, 6, 7), 3.165, NUMS, seed=77)
    n = len(atoms)
    e_o, f_o, v_o = O.evaluate(ob, atoms, coeff, virial=True)
    calc = calculator.UFCalculator(model, md_skin=0.0)
    for _ in range(2):
        calc.evaluate_frames([atoms], virial=True)
    dbg.launches()
    for world in (3, 8):
        for which in ("atoms", "centres"):
            share = calc.evaluate_atom_range if which == "atoms" else calc.evaluate_centre_range
            parts = [share(atoms, *parallel.shard_range(n, r, world), virial=True) for r in range(world)]
            said = dbg.launches()
            assert len(said) >= world and all(s["vir"] == 1 and s["centres"] == int(which == "centres") for s in said), said
            assert all(s["gather"] == int(which == "atoms") for s in said), said
            _check_frame(sum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts), ob, atoms, coeff,
                         f"{which} x {world}")
    monkeypatch.setenv("UF3_NO_HALO", "1")
    parts = [calc.evaluate_centre_range(atoms, *parallel.shard_range(n, r, 3), virial=True) for r in range(3)]
    monkeypatch.delenv("UF3_NO_HALO")
    _check_frame(sum(p[0] for p in parts), sum(p[1] for p in parts), sum(p[2] for p in parts), ob, atoms, coeff, "no halo")
    e1, f1, v1 = parallel.sharded_evaluate(calc, atoms, virial=True)
    _check_frame(e1, f1, v1, ob, atoms, coeff, "sharded_evaluate")
    ev = parallel.ShardedEvaluator(calc, atoms, md_skin=0.5)
    try:
        assert ev.device_route and not ev.decomposed
        e, f, v = ev.step().result()
        _check_frame(e, f, v, ob, atoms, coeff, "ShardedEvaluator")
        rng = np.random.default_rng(9)
        for step in range(3):
            ev.positions.add_(torch.from_numpy(rng.uniform(-0.02, 0.02, (n, 3))).to(ev.positions.device))
            e, f, v = ev.step().result()
            moved = _frame(atoms, positions=ev.host_positions())
            _check_frame(e, f, v, ob, moved, coeff, f"ShardedEvaluator step {step}")
        said = dbg.launches()
        assert said[-1]["md"] == 1 and said[-1]["vir"] == 1, said
    finally:
        ev.close()


@pytest.mark.parametrize("which", ["primitive", "triclinic"])
def test_stress_surface(which, dbg):
    """UFCalculator._get_stress: the analytic strain derivative over the volume against the oracle's, and against the
    calculator's own finite-difference route (numerical=True, the reference's, calculator.py:399-404)."""
    basis = dbg.basis(synthetic.notebook_basis(MOW))
    model, coeff = _model(basis, 61)
    atoms = _small_frames()[which]
    calc = calculator.UFCalculator(model, md_skin=0.0)
    stress = calc._get_stress(atoms)
    _, _, v_o = O.evaluate(O.OracleBasis(basis), atoms, coeff, virial=True)
    vol = abs(np.linalg.det(np.asarray(atoms.get_cell(), dtype=float).reshape(3, 3)))
    assert worst_elementwise(stress, v_o / vol, rtol=1e-9, floor=1e-11) <= 1.0, (stress, v_o / vol)
    numeric = calc._get_stress(atoms, numerical=True)
    assert np.abs(stress - numeric).max() <= 1e-7 * np.abs(numeric).max(), (stress, numeric)


def test_cw_lanes_without_a_triplet_stay_finite_when_two_neighbours_coincide(dbg, monkeypatch):
    """Two atoms at one point (a 5 x 5 x 5 rattled bcc W cell plus a copy of atom 0): every centre near them has two entries at
    one point in its 3-body list, whose would-be triplet has a leg of length 0.  The oracle drops every term with such a leg
    (trio r_min 1.5, pair r_min 0.001), so its results are finite.  In the CW instances every lane takes part in the force
    gather, a lane without a triplet included: it must carry zeros, not 0 * (1 / 0).  The MD route (skin 0.5, lists of at most
    16 entries: CW runs) against UF3_EVAL_NO_CW, the plain route and the oracle."""
    basis = dbg.basis(synthetic.notebook_basis(['W']))
    model, coeff = _model(basis, 71)
    ob = O.OracleBasis(basis)
    base = synthetic.lattice_frame("bcc", (5, 5, 5), 3.165, [74], seed=72)
    pos = np.vstack([base.get_positions(), base.get_positions()[:1]])
    atoms = Atoms(numbers=[74] * len(pos), positions=pos, cell=base.get_cell(), pbc=True)
    plain = calculator.UFCalculator(model, md_skin=0.0)
    for _ in range(2):
        ref = plain.evaluate_frames([atoms], virial=True)
    md = calculator.UFCalculator(model, md_skin=0.5)
    dbg.launches()
    for _ in range(2):
        got = md.evaluate_frames([atoms], virial=True)
    said = dbg.launches()
    assert said[-1]["md"] == 1 and said[-1]["cw"] == 1 and said[-1]["cap"] <= 16, said
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all() and np.isfinite(got[3]).all()
    monkeypatch.setenv("UF3_EVAL_NO_CW", "1")
    nocw = md.evaluate_frames([atoms], virial=True)
    said = dbg.launches()
    monkeypatch.delenv("UF3_EVAL_NO_CW")
    assert said[-1]["md"] == 1 and said[-1]["cw"] == 0, said
    for other in (nocw, ref):
        assert abs(got[0][0] - other[0][0]) <= 1e-12 * abs(other[0][0])
        assert np.abs(got[1] - other[1]).max() <= 1e-12 * np.abs(other[1]).max()
        assert worst_elementwise(got[3], other[3], rtol=1e-10, floor=1e-11) <= 1.0
    _check_batch(got, ob, [atoms], coeff, "coincident atoms")
