"""
Every kernel route on equivalent descriptions of one crystal (tests/_util.py: equivalence_cases; the oracle satisfies the same
relations in tests/test_oracle_invariance.py): strongly skewed re-descriptions whose bin radius exceeds the bin count and whose
runs wrap more than once along the fast axis, supercells, a 1-atom primitive cell against its conventional cell, permutations,
rotations and translations; bulk, slab and wire; two, three and five species; frames of each size class of the cell-list stage
(one cell <= 256 atoms, one workgroup <= 2048, the general stage beyond, and UF3_NO_SMALL_PREPARE for small frames).

On each description the featurizer's launch families and every evaluator route are held to the oracle on that description and
to the original through the description's mapping, entry by entry; forces to minus the gradient of the same route's energy.
"""
import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic, _lib
from uf3_amd.data import analyze
from uf3_amd.forcefield import calculator
from uf3_amd.regression import least_squares as ls
from uf3_amd.representation import process
from _util import dbg, describe, equivalence_cases, worst_elementwise, wrapped  # noqa: F401  (dbg: the fixture)
from test_gpu_analyze import restated
from test_gpu_virial import _MD_ROUTES

pytestmark = pytest.mark.gpu
TOL = 1e-9                  # rows, energies and forces: relative, entry by entry
FD_TOL = 1e-8               # max |F - F_fd| <= FD_TOL * max |F|
H = (1e-4, 5e-5)            # Richardson pair
CASES = equivalence_cases()
FD_CASES = [("bcc_mow", "skew_821"), ("bcc_mow", "skew_751_reflection"), ("slab_mow", "skew_in_plane_531"),
            ("slab_ghost_terms", "skew_in_plane_131"), ("wire_mow", "perm_rotation_shift"), ("quinary", "skew_351")]
FD_PICKS = [(a, c) for a in (0, 3, 6, 9, 12, 15) for c in range(3)]
# launch families of the featurizer: environment, what featurizer_modes must say (bits 12: k_featurize3, 6-9: matrix cores,
# 1-5: generic), and whether the k_featurize3 debug line must appear
FAMILIES = {
    "feat3": ({}, lambda m: bool(m & 0x1000), True),
    "feat3_general_stage": ({"UF3_NO_SMALL_PREPARE": "1"}, lambda m: bool(m & 0x1000), True),
    "matrix_core": ({"UF3_NO_FEAT3": "1"}, lambda m: bool(m & 0x3c0) and not m & 0x1000, False),
    "generic": ({"UF3_NO_FEAT3": "1", "UF3_NO_MFMA_FEAT": "1"}, lambda m: bool(m & 0x3e) and not m & 0x3c0 and not m & 0x1000,
                False),
}
_ORACLE, _ORACLE_EFV, _LARGE = {}, {}, []


def _large():
    """name, (elements, frame, [Description]) of a frame of > 2048 atoms (the general cell-list stage) and a skewed description"""
    if not _LARGE:
        big = wrapped(synthetic.lattice_frame("bcc", (9, 9, 13), 3.165, [42, 74], seed=88))
        _LARGE.append(("large", (["Mo", "W"], big, [describe(big, "skew_321", U=[[1, 0, 0], [0, 1, 0], [3, 2, 1]])])))
    return _LARGE[0]


def _oracle_efv(ob, case, d, atoms, coeff):
    """the oracle's energy, forces and strain derivative (the same on every route: computed once per description)"""
    key = (case, d.label if d is not None else None)
    if key not in _ORACLE_EFV:
        _ORACLE_EFV[key] = O.evaluate(ob, atoms, coeff, virial=True)
    return _ORACLE_EFV[key]


def _oracle_rows(els, lead3, case, d):
    key = (case, lead3, d.label if d is not None else None)
    if key not in _ORACLE:
        ob = O.OracleBasis(synthetic.notebook_basis(els, lead3=lead3))
        _ORACLE[key] = O.featurize(ob, CASES[case][1] if d is None else d.atoms)
    return _ORACLE[key]


def _rows_close(got, want, label, scale=None):
    """entry by entry within TOL; rows that vanish by symmetry (force rows of the perfect primitive crystal) within 1e-12 of
    ``scale`` (the energy row's largest entry)"""
    want = np.asarray(want)
    if scale is not None and np.abs(want).max() <= 1e-12 * scale:
        assert np.abs(got).max() <= 1e-12 * scale, label
    else:
        w = worst_elementwise(got, want, rtol=TOL, floor=1e-12)
        assert w <= 1.0, (label, w)


@pytest.fixture
def fresh(monkeypatch, capfd):
    """featurizers on a fresh context made with UF3_DEBUG_LDS, whose device tables are built under the given environment"""
    monkeypatch.setenv("UF3_DEBUG_LDS", "1")
    monkeypatch.setattr(_lib, "_contexts", {})
    made = []

    def make(basis, env):
        for k in ("UF3_NO_FEAT3", "UF3_NO_MFMA_FEAT", "UF3_NO_SMALL_PREPARE"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        _lib.drop_device_basis(basis)
        made.append(basis)
        fz = process.BasisFeaturizer(basis)
        return fz, fz._dev()[1].featurizer_modes

    def feat3_lines():
        return sum(line.startswith("uf3 featurize3:") for line in capfd.readouterr().err.splitlines())

    make.feat3_lines = feat3_lines
    yield make
    for b in made:
        _lib.drop_device_basis(b)


def _rows(fz, atoms):
    x_e, x_f, _ = fz.featurize_frames([atoms])
    e_only = fz.featurize_frames([atoms], forces=False)[0]
    f_only = fz.featurize_frames([atoms], energy=False)[1]
    return x_e[0], x_f, e_only[0], f_only


@pytest.mark.parametrize("lead3", [3, 0])
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("case", list(CASES))
def test_feature_rows_of_equivalent_descriptions(case, family, lead3, fresh):
    """Each description one frame per call (its own size class), with energy and forces, energy only and forces only: against
    the oracle on the description and against the original's rows through the mapping."""
    els, base, descs = CASES[case]
    env, modes_ok, feat3 = FAMILIES[family]
    basis = synthetic.notebook_basis(els, lead3=lead3)
    fz, modes = fresh(basis, env)
    assert modes_ok(modes), (family, hex(modes))
    fresh.feat3_lines()
    x_e0, x_f0, _, _ = _rows(fz, base)
    ref0 = _oracle_rows(els, lead3, case, None)
    scale = np.abs(ref0["xe"]).max()
    _rows_close(x_e0, ref0["xe"], (case, "original", "energy row"))
    _rows_close(x_f0, ref0["xf"], (case, "original", "force rows"), scale)
    for d in descs:
        x_e, x_f, e_only, f_only = _rows(fz, d.atoms)
        ref = _oracle_rows(els, lead3, case, d)
        for what, got in (("energy row", x_e), ("energy-only row", e_only)):
            _rows_close(got, ref["xe"], (case, d.label, what))
            _rows_close(got, d.xe(x_e0), (case, d.label, what, "mapped"))
        for what, got in (("force rows", x_f), ("forces-only rows", f_only)):
            _rows_close(got, d.xf(x_f0), (case, d.label, what, "mapped"), scale)
            if d.reference_drops_terms:     # (the kernels keep the ghost-centred terms the reference drops: DESIGN.md section 7)
                assert worst_elementwise(got, ref["xf"]) > 1e3, (case, d.label, what)
            else:
                _rows_close(got, ref["xf"], (case, d.label, what), scale)
    lines = fresh.feat3_lines()
    assert (lines > 0) == feat3, (family, lines)


def test_large_frame_and_a_skewed_description(fresh):
    """> 2048 atoms: k_frame_bins, k_scan_small, k_bin_fill, k_bin_finish.  The skewed description against the oracle, the
    original against the skewed one through the mapping, on the k_featurize3 launch and on the generic one."""
    _, (_, big, (d,)) = _large()
    assert len(big) > 2048
    basis = synthetic.notebook_basis(["Mo", "W"])
    ref = O.featurize(O.OracleBasis(basis), d.atoms)
    rows = {}
    for family in ("feat3", "generic"):
        env, modes_ok, _ = FAMILIES[family]
        fz, modes = fresh(basis, env)
        assert modes_ok(modes), (family, hex(modes))
        x_e0, x_f0, _ = fz.featurize_frames([big])
        x_e, x_f, _ = fz.featurize_frames([d.atoms])
        _rows_close(x_e[0], ref["xe"], (family, "energy row"))
        _rows_close(x_f, ref["xf"], (family, "force rows"))
        _rows_close(x_e[0], d.xe(x_e0[0]), (family, "energy row", "mapped"))
        _rows_close(x_f, d.xf(x_f0), (family, "force rows", "mapped"))
        rows[family] = x_f0
    _rows_close(rows["feat3"], rows["generic"], "feat3 vs generic")


@pytest.mark.parametrize("case,label", [("bcc_mow", "skew_821"), ("slab_ghost_terms", "skew_in_plane_131")])
def test_energy_row_gradient_is_the_force_rows_on_a_skewed_cell(case, label, fresh):
    """-d x_e / d r = x_f on the [8, 2, 1] description and on the slab description where the reference drops ghost-centred
    terms (the kernels keep them): Richardson differences of the k_featurize3 launch's energy rows"""
    els, _, descs = CASES[case]
    atoms = next(d for d in descs if d.label == label).atoms
    fz, modes = fresh(synthetic.notebook_basis(els), {})
    assert modes & 0x1000
    x_f = fz.featurize_frames([atoms])[1]
    frames, picks = [], FD_PICKS[::4]
    for a, c in picks:
        for h in H:
            for sgn in (1, -1):
                p = atoms.get_positions()
                p[a, c] += sgn * h
                frames.append(type(atoms)(numbers=atoms.get_atomic_numbers(), positions=p, cell=atoms.get_cell(), pbc=atoms.get_pbc()))
    x_e = fz.featurize_frames(frames, forces=False)[0].reshape(len(picks), 2, 2, -1)
    d = -(x_e[:, :, 0] - x_e[:, :, 1]) / (2 * np.array(H))[None, :, None]
    fd = (4 * d[:, 1] - d[:, 0]) / 3
    assert fresh.feat3_lines() > 0
    for k, (a, c) in enumerate(picks):
        assert np.abs(fd[k] - x_f[a, c]).max() <= FD_TOL * np.abs(x_f).max(), (a, c)


def _model(basis, seed):
    model = ls.WeightedLinearModel(basis)
    coeff = np.random.default_rng(seed).normal(0, 0.05, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    model.coefficients = coeff
    return model, coeff


def _efv(calc, atoms):
    e, f, _, v = calc.evaluate_frames([atoms], virial=True)
    return e[0], f, v[0]


def _check_efv(got, want, label, f_scale):
    e, f, v = got
    e_w, f_w, v_w = want
    assert abs(e - e_w) <= TOL * abs(e_w), (label, e, e_w)
    assert worst_elementwise(v, v_w, rtol=TOL, floor=1e-11) <= 1.0, (label, v, v_w)
    if f_w is not None:
        if np.abs(f_w).max() <= 1e-12 * f_scale:
            assert np.abs(f).max() <= 1e-12 * f_scale, label
        else:
            assert worst_elementwise(f, f_w, TOL) <= 1.0, label


def _route_flags(want, els):
    """what the debug line must say on a route; the five-species basis runs every route without the TAB instances"""
    return {k: v for k, v in want.items() if not (k == "tab" and len(els) > 3)}


@pytest.mark.parametrize("route", list(_MD_ROUTES))
def test_evaluator_routes_on_equivalent_descriptions(route, dbg, monkeypatch):
    """Energy, forces and strain derivative of every description on the route: against the oracle on the description, against
    the route's own results on the original through the mapping, forces adding up to zero; on a fresh MD calculator (skin 0.5)
    per description whose launches say the route ran."""
    env, want0 = _MD_ROUTES[route]
    large, big = _large()
    for case, (els, base, descs) in {**CASES, large: big}.items():
        want = _route_flags(want0, els)
        basis = dbg.basis(synthetic.notebook_basis(els))
        model, coeff = _model(basis, 17)
        ob = O.OracleBasis(basis)
        for k in env:
            monkeypatch.delenv(k, raising=False)
        plain = calculator.UFCalculator(model, md_skin=0.0)
        for _ in range(2):                                           # (list capacities tuned: the MD route starts from a tuned context)
            for a in [base] + [d.atoms for d in descs]:
                plain.evaluate_frames([a], virial=True)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        dbg.launches()
        results = {}
        for d in [None] + descs:
            atoms = base if d is None else d.atoms
            calc = calculator.UFCalculator(model, md_skin=0.5)
            first = _efv(calc, atoms)
            second = _efv(calc, atoms)
            said = dbg.launches()
            assert said and said[-1]["vir"] == 1, said
            for key, val in want.items():
                assert said[-1][key] == val, (route, case, d and d.label, said)
            results[d.label if d else None] = second
            label = (route, case, d.label if d else "original")
            e0, f0, v0 = _oracle_efv(ob, case, d, atoms, coeff)
            f_scale = abs(e0)
            drops = d is not None and d.reference_drops_terms
            for got in (first, second):
                _check_efv(got, (e0, None if drops else f0, v0), label + ("oracle",), f_scale)
                if drops:                   # (the kernels keep the ghost-centred terms the reference drops: DESIGN.md section 7)
                    assert np.abs(got[1] - f0).max() > 1e-6 * np.abs(f0).max(), label
            if d is not None:
                b = results[None]
                _check_efv(second, (d.energy(b[0]), d.forces(b[1]), d.virial(b[2])), label + ("mapped",), f_scale)
            f = second[1]
            assert np.abs(f.sum(axis=0)).max() <= 1e-11 * max(1.0, np.abs(f).max()), label


@pytest.mark.parametrize("route", list(_MD_ROUTES))
def test_evaluator_forces_are_minus_the_gradient_of_its_energy(route, dbg, monkeypatch):
    """Richardson differences of the route's own energy (h = 1e-4, 5e-5) for 6 atoms x 3 components of skewed cells, slab and
    wire: on the MD route these are steps inside the skin (the persistent lists serve every one)."""
    env, want0 = _MD_ROUTES[route]
    report = []
    for case, label in FD_CASES:
        els, _, descs = CASES[case]
        want = _route_flags(want0, els)
        atoms = next(d for d in descs if d.label == label).atoms
        basis = dbg.basis(synthetic.notebook_basis(els))
        model, _ = _model(basis, 23)
        for k in env:
            monkeypatch.delenv(k, raising=False)
        plain = calculator.UFCalculator(model, md_skin=0.0)
        for _ in range(2):
            plain.evaluate_frames([atoms], virial=True)
        for k, val in env.items():
            monkeypatch.setenv(k, val)
        calc = calculator.UFCalculator(model, md_skin=0.5)
        _, f, _ = _efv(calc, atoms)
        dbg.launches()
        fd = []
        for a, c in FD_PICKS:
            d = []
            for h in H:
                es = []
                for sgn in (1, -1):
                    p = atoms.get_positions()
                    p[a, c] += sgn * h
                    es.append(_efv(calc, type(atoms)(numbers=atoms.get_atomic_numbers(), positions=p, cell=atoms.get_cell(),
                                                     pbc=atoms.get_pbc()))[0])
                d.append(-(es[0] - es[1]) / (2 * h))
            fd.append((4 * d[1] - d[0]) / 3)
        said = dbg.launches()
        assert len(said) >= 4 * len(FD_PICKS), len(said)
        for key, val in want.items():
            assert all(s[key] == val for s in said), (route, case, label, key, said[:3])
        got = np.array([f[a, c] for a, c in FD_PICKS])
        err = np.abs(got - np.array(fd)).max() / np.abs(f).max()
        report.append(f"{route} {case} {label}: max |F - F_fd| / max |F| = {err:.2e}")
        assert err <= FD_TOL, (route, case, label, err)
    print("\n".join(report))


@pytest.mark.parametrize("case", ["bcc_mow", "slab_mow", "wire_mow", "bcc_w_primitive", "large"])
def test_pair_histograms_of_equivalent_descriptions(case):
    """uf3_pair_histogram on the skewed and supercell descriptions: equal to the NumPy restatement of the reference, and each
    species pair's total n times the original's (once for a re-description)"""
    els, base, descs = _large()[1] if case == "large" else CASES[case]
    species = sorted(set(int(z) for z in base.get_atomic_numbers()))
    edges = np.linspace(0, 6.0, 601)
    got0, _ = analyze.pair_histograms([base], species, edges, 0.0, 6.0, upper_inclusive=True)
    np.testing.assert_array_equal(got0, restated(base, species, edges, 6.0, True))
    for d in descs:
        got, _ = analyze.pair_histograms([d.atoms], species, edges, 0.0, 6.0, upper_inclusive=True)
        np.testing.assert_array_equal(got, restated(d.atoms, species, edges, 6.0, True), err_msg=d.label)
        assert np.array_equal(got.sum(axis=1), d.scale * got0.sum(axis=1)), (d.label, got.sum(axis=1), got0.sum(axis=1))
