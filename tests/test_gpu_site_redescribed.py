"""Site rows, the fused grade kernel, the per-frame maximum, the in-MD grade samples and per-atom leverages on re-described
frames (uf3_site_rows, uf3_site_grade, uf3_md_run_grade, uf3_leverage through UFCalculator.get_leverages).

The frames are those of tests/test_redescribed_host.py (image ranges [8, 2, 1], [3, 5, 1] and [7, 5, 1], reflections,
permutations, a slab, a wire, the 1-atom primitive cell, five and eight species, supercells of 128, 216 and 432 atoms, atoms
outside their cell); tests/test_site_redescribed_host.py pins the host rows, the posteriors and what the references alone spread
by, and this module imports them.

1. rows against the host rows of every pinned description;
2. symmetry-1 bases on skewed and turned descriptions: there the supercell-index tie-break decides the COLUMN of a product (the
   host module shows rows that differ from the mapped original's by 2.5e-2 and more while their sums agree);
3. the five- and eight-species bases (F = 5675 / 8164, rows of 45 and 65 KB in LDS) through coefficients and column sums; no
   grades there: a posterior of that size is a 0.25 to 0.5 GB W;
4. device against device through every description's mapping;
5. a batch of unlike cells, bit for bit what every frame gets alone, on both grade routes;
6. leverages under the mappings;
7. atoms outside their cell (include/uf3_hip.h: "an atom outside its cell counts as its image inside");
8. grade samples inside MD on a re-described cell.

Bounds, none of them new: rows 1e-10 of the largest |B| (tests/test_gpu_site_grade.py: RTOL); grades ``ls.leverage_bound``
against ``ls.leverage_reference`` of the device's own rows (_check_grades); leverages tests/test_gpu_leverage.py: _within.
Across descriptions: max(100 x the spread of the references alone (the host module's HOST_SPREAD / MD_HOST_SPREAD), the sum of
the two results' ``leverage_bound``) -- 100 being the ratio of the README's row parity (1e-13) to the oracle's own spread across
descriptions (1e-14 to 1e-15), which the same W amplifies alike."""
import ctypes as C
import functools
import gc
import re

import numpy as np
import pytest

from uf3_amd import _lib, pipeline, synthetic
from uf3_amd.forcefield import calculator
from uf3_amd.forcefield.md import MolecularDynamics
from uf3_amd.regression import least_squares as ls
from uf3_amd.representation import process
import _flux_ref as FR
import _site_rows_ref as SR
import _uneven as UN
import test_redescribed_host as RH
import test_site_redescribed_host as SH
from _util import wrapped
from test_gpu_leverage import _within
from test_gpu_site_grade import RTOL, _check_grades, _grades, _rows, _sub

pytestmark = pytest.mark.gpu

ORIGINAL = RH.ORIGINAL
SPREAD_FACTOR = 100.0
_ids = lambda pairs: [f"{c}-{l}" for c, l in pairs]                       # noqa: E731


def _report(what, **figures):
    print(what + ": " + ", ".join(f"{k} {v:.2e}" if isinstance(v, float) else f"{k} {v}" for k, v in figures.items()))


# ============================================================================================ 1. rows against the host rows
@pytest.mark.parametrize("case,label", SH.ROWS_HARD, ids=_ids(SH.ROWS_HARD))
def test_rows_against_the_host_rows(case, label):
    basis, atoms = RH.basis(case), RH.frame(case, label)
    B = SH.host_rows(case, label)
    got = _rows(basis, [atoms])
    err = float(np.abs(got - B).max() / np.abs(B).max())
    _report(f"{case} {label}: rows against the host rows", F=basis.n_feats, error=err, bound=RTOL)
    assert err <= RTOL
    assert np.array_equal(got, _rows(basis, [atoms]))                   # the same call twice


# ======================================================================================= 2. symmetry-1 bases, skewed and turned
SYM1_PICKS = [(name, label) for name, (_, labs) in SH.SYM1.items() for label in labs]


@pytest.mark.parametrize("name,label", SYM1_PICKS, ids=_ids(SYM1_PICKS))
def test_symmetry_1_rows_and_grades_on_skewed_and_turned_descriptions(name, label):
    """Against THAT description's host rows: the original's rows through ``src`` are another matrix here, by 2.5e-2 to 1.8e-1 of
    an entry (the host module's floor), while the sums of the rows -- every energy-level check -- cannot tell.  In the one-atom
    cell every neighbour is an image of the centre: the order of the images alone decides every column."""
    case = SH.SYM1[name][0]
    basis, atoms = SH.sym1_basis(name), RH.frame(case, label)
    B = SH.sym1_rows(name, label)
    got = _rows(basis, [atoms])
    err = float(np.abs(got - B).max() / np.abs(B).max())
    _report(f"{name} on {case} {label}: rows against this description's host rows", error=err, bound=RTOL)
    assert err <= RTOL
    assert np.array_equal(got, _rows(basis, [atoms]))
    _check_grades(basis, [atoms], SH.sym1_whitening(name), f"{name} {case} {label}")


# =============================================================================== 3. five and eight species: coefficients, sums
LARGE = [("quinary", "skew_351"), ("quinary", "perm_rotation"), (RH.S8, ORIGINAL)]
LARGE_SEEDS = [201, 202, 203, 204]


@functools.lru_cache(maxsize=None)
def _large_rows(case, label):
    rows = _rows(RH.basis(case), [RH.frame(case, label)])
    rows.setflags(write=False)
    return rows


def _seeded_coefficients(basis, seed):
    """RH.model's recipe with another seed"""
    c = np.random.default_rng(seed).normal(0, 0.05, basis.n_feats)
    c[np.asarray(basis.col_idx, dtype=int)] = 0.0
    n_el = len(basis.element_list)
    c[:n_el] = np.linspace(-0.3, 0.2, n_el)
    return c


@pytest.mark.parametrize("seed", LARGE_SEEDS)
@pytest.mark.parametrize("case,label", LARGE, ids=_ids(LARGE))
def test_large_bases_through_coefficients(case, label, seed):
    basis, atoms = RH.basis(case), RH.frame(case, label)
    c = _seeded_coefficients(basis, seed)
    U = FR.site_terms(RH.oracle_basis(case), atoms, c)[0]
    err = RH.rel(_large_rows(case, label) @ c, U)
    _report(f"{case} {label} seed {seed}: rows @ c against the restatement's U", F=basis.n_feats, error=err, bound=RTOL)
    assert err <= RTOL


@pytest.mark.parametrize("case,label", LARGE, ids=_ids(LARGE))
def test_large_bases_column_sums_and_the_one_body_columns(case, label):
    """F = 5675 and 8164: the row in LDS is 8 site_row_stride(F) = 45 584 and 65 552 bytes; pair_col, trio_of and lut with five
    and eight species.  No grades: a posterior of this size is not feasible in a test."""
    basis, atoms = RH.basis(case), RH.frame(case, label)
    rows = _large_rows(case, label)
    x_e, live = SH.energy_row(RH.oracle_basis(case), atoms), SH.live_columns(basis)
    err = np.abs(rows.sum(0) - x_e)[live] / np.abs(x_e).max()
    _report(f"{case} {label}: live-column sums against the oracle's energy row", F=basis.n_feats, columns=int(np.count_nonzero(x_e)),
            error=float(err.max()), bound=RTOL)
    assert np.all(err <= RTOL), int(np.argmax(err))
    zs = [int(q) for q in RH.oracle_basis(case).species_z]
    n_el = len(zs)
    want = np.zeros((len(atoms), n_el))
    want[np.arange(len(atoms)), [zs.index(int(q)) for q in atoms.get_atomic_numbers()]] = 1.0
    assert np.array_equal(rows[:, :n_el], want)
    assert np.array_equal(rows, _rows(basis, [atoms]))


# ======================================================================================= 4. device against device, by mapping
MAPPED = [c for c in RH.CASES if RH.CASES[c][1] and RH.basis(c).n_feats <= SH.MAX_ROWS_FEATS]


@functools.lru_cache(maxsize=None)
def _whitening(case):
    return SH.whitening(case) if case in SH.LEVERAGE_CASES else SH._frozen(SR.seeded_model(RH.basis(case)).whitening().copy())


@pytest.mark.parametrize("case", MAPPED)
def test_rows_grades_and_the_maximum_through_the_mappings(case):
    basis, w = RH.basis(case), _whitening(case)
    B0, g0 = _check_grades(basis, [RH.frame(case, ORIGINAL)], w, f"{case} original")
    _, fm0, fa0 = _grades(basis, [RH.frame(case, ORIGINAL)], w)
    b0 = ls.leverage_bound(B0, w, 1)
    worst = dict(rows=0.0, grades_over_bound=0.0)
    sizes = []
    for label in RH.labels(case)[1:]:
        d = RH.description(case, label)
        B, g = _check_grades(basis, [d.atoms], w, f"{case} {label}")       # (frame_max == max of the call's grades, bit for bit)
        worst["rows"] = max(worst["rows"], float(np.abs(B - B0[d.src]).max() / np.abs(B0).max()))
        # grades of two descriptions: each within its bound of the reference of its own rows, the references within the host
        # spread (where the host module measured one)
        if case in SH.HOST_SPREAD:
            tol = np.maximum(ls.leverage_bound(B, w, 1) + b0[d.src], SPREAD_FACTOR * SH.HOST_SPREAD[case]["grade"] * g0.max())
            over = float((np.abs(g - g0[d.src]) / tol).max())
            worst["grades_over_bound"] = max(worst["grades_over_bound"], over)
            assert over <= 1.0, (case, label, over)
        _, fm, fa = _grades(basis, [d.atoms], w)
        assert fm[0] == g.max()
        if case in SH.ARGMAX_CASES:
            assert d.src[fa[0]] == fa0[0], (case, label, fa[0], d.src[fa[0]], fa0[0])
        sizes.append(len(d.atoms))
    _report(f"{case}: rows, grades through the mappings, frames of {sizes} atoms", **worst, rows_bound=RTOL)
    assert worst["rows"] <= RTOL
    assert fm0[0] == g0.max()


def test_the_mapped_frames_hold_the_large_supercells_and_the_wire():
    sizes = sorted(len(d.atoms) for c in MAPPED for d in RH.CASES[c][1])
    assert {108, 128, 216, 432} <= set(sizes), sizes


# ======================================================================================================= 5. a batch of unlike cells
BATCH = [("bcc_mow", "skew_821"), ("slab_mow", "skew_in_plane_531"), ("wire_mow", ORIGINAL), ("bcc_mow", "supercell_222_skew_821")]


@pytest.fixture
def report(monkeypatch, capfd):
    """A fresh context that reports its launches (tests/test_gpu_site_grade.py: report) and two bases of the test's own, whose
    device tables live and die with it: ``(read, notebook Mo/W basis, sym1_binary)``; ``read()`` returns (and clears) the
    site-grade launches since the last look."""
    monkeypatch.setenv("UF3_DEBUG_LDS", "1")
    monkeypatch.setattr(_lib, "_contexts", {})
    bases = [synthetic.notebook_basis(["Mo", "W"]), UN.sym1_binary()]

    def read():
        err = capfd.readouterr().err
        return [dict(kv.split("=") for kv in m.group(1).split() if "=" in kv) for m in re.finditer(r"uf3: site grade (.*)", err)]
    yield (read,) + tuple(bases)
    for b in bases:
        _lib.drop_device_basis(b)
    gc.collect()


def _grades_with_an_empty_frame(basis, frames, w, at):
    """uf3_site_grade on ``frames`` with a frame without atoms put in front of frame ``at`` (whose cell and pbc it is given)"""
    ctx = _lib.get_context(None)
    db = _lib.device_basis(basis, ctx)
    batch = _lib.FrameBatch(list(frames))
    off = np.ascontiguousarray(np.insert(batch.offsets, at, batch.offsets[at]), dtype=np.int64)
    cells = np.ascontiguousarray(np.insert(batch.cells, at, batch.cells[at], axis=0))
    pbc = np.ascontiguousarray(np.insert(batch.pbc, at, batch.pbc[at], axis=0))
    fr = _lib.make_frames(off, cells, pbc)
    w = np.ascontiguousarray(w, dtype=np.float64)
    n = len(off) - 1
    g, fm, fa = np.empty(batch.n_atoms), np.full(n, np.nan), np.full(n, 7, dtype=np.int32)
    ctx.check(ctx.lib.uf3_site_grade(db.handle, C.byref(fr), _lib._p(batch.pos), _lib._p(batch.z), _lib._p(w), _lib._p(g), _lib._p(fm),
                                     _lib._p(fa)))
    return g, fm, fa


def test_a_batch_of_unlike_cells_gives_each_frame_what_it_gets_alone(report):
    """A skewed bulk cell, a skewed slab, a wire and a skewed 128-atom supercell in one call, then with a 15-atom frame in front:
    every 16-row tile of k_site_grade then straddles two frames with different cells and pbc."""
    read, mow, sym1 = report
    frames = [RH.frame(c, l) for c, l in BATCH]
    assert [len(a) for a in frames] == [16, 16, 36, 128]
    assert mow.n_feats == 434 and sym1.n_feats == 983 > 608
    for basis, kernel in ((mow, "k_site_grade"), (sym1, "k_site_rows+k_leverage")):
        w = SR.seeded_model(basis).whitening()
        alone = [(_rows(basis, [a]),) + _grades(basis, [a], w) for a in frames]
        read()
        for front in ([], [_sub(frames[0], 15)]):
            batch = front + frames
            nf = len(front)
            off = np.concatenate([[0], np.cumsum([len(a) for a in batch])])
            rows = _rows(basis, batch)
            g, fm, fa = _grades(basis, batch, w)
            launches = read()
            assert launches and all(d["kernel"] == kernel and d["feat"] == str(basis.n_feats) for d in launches), launches
            for k in range(len(frames)):
                kk = k + nf
                assert np.array_equal(rows[off[kk]:off[kk + 1]], alone[k][0]), (kernel, nf, k)
                assert np.array_equal(g[off[kk]:off[kk + 1]], alone[k][1]), (kernel, nf, k)
                assert fm[kk] == alone[k][2][0] and fa[kk] == alone[k][3][0], (kernel, nf, k)
            # the grade entry with an empty frame in the middle: 0 and -1 there, nothing else moves
            at = nf + 2
            ge, fme, fae = _grades_with_an_empty_frame(basis, batch, w, at)
            assert np.array_equal(ge, g)
            assert fme[at] == 0.0 and fae[at] == -1
            assert np.array_equal(np.delete(fme, at), fm) and np.array_equal(np.delete(fae, at), fa)
            read()


# ============================================================================================ 6. leverages under the mappings
@functools.lru_cache(maxsize=None)
def _calc(case):
    return calculator.UFCalculator(SH.posterior(case), md_skin=0.0)


@pytest.mark.parametrize("case", SH.LEVERAGE_CASES)
def test_leverages_through_the_mappings(case):
    """get_leverages with force rows.  Its energy leverage is that of the per-atom energy row x_e / N; times N^2 it is the raw
    row's, which scales with scale^2.  The per-atom force leverage sums the three force rows of an atom: invariant under an
    orthogonal Q -- the group = 3 path of k_leverage on real rows."""
    calc, basis, w = _calc(case), RH.basis(case), SH.whitening(case)
    fz = process.BasisFeaturizer(basis)
    spread = SH.HOST_SPREAD[case]
    res = {}
    for label in RH.labels(case, RH.MAX_RESTATED):
        atoms = RH.frame(case, label)
        out = calc.get_leverages([atoms])
        x_e, x_f, _ = fz.featurize_frames([atoms])
        x_e, x_f = x_e / len(atoms), x_f.reshape(-1, x_f.shape[-1])
        _within(out["energy"], x_e, w, 1, f"{case} {label}: energy leverage, group 1")
        _within(out["force"], x_f, w, 3, f"{case} {label}: per-atom force leverage, group 3")
        n2 = float(len(atoms)) ** 2
        res[label] = (out["energy"][0] * n2, ls.leverage_bound(x_e, w, 1)[0] * n2, out["force"], ls.leverage_bound(x_f, w, 3))
    e0, be0, f0, bf0 = res[ORIGINAL]
    worst = dict(energy_over_bound=0.0, force_over_bound=0.0)
    for label in RH.labels(case, RH.MAX_RESTATED)[1:]:
        d = RH.description(case, label)
        e, be, f, bf = res[label]
        tol_e = max(SPREAD_FACTOR * spread["energy"] * d.scale ** 2 * e0, be + d.scale ** 2 * be0)
        tol_f = np.maximum(SPREAD_FACTOR * spread["force"] * f0.max(), bf + bf0[d.src])
        over_e, over_f = abs(e - d.scale ** 2 * e0) / tol_e, float((np.abs(f - f0[d.src]) / tol_f).max())
        assert over_e <= 1.0 and over_f <= 1.0, (case, label, over_e, over_f)
        worst = dict(energy_over_bound=max(worst["energy_over_bound"], over_e), force_over_bound=max(worst["force_over_bound"], over_f))
    _report(f"{case}: leverages across {len(res) - 1} descriptions", **worst, energy_bound_rel=float(max(SPREAD_FACTOR * spread["energy"], 2 * be0 / e0)),
            force_bound_rel=float(max(SPREAD_FACTOR * spread["force"], 2 * np.median(bf0 / f0))))


# ================================================================================================ 7. atoms outside their cell
UNWRAPPED = ["one_atom", "every_atom"]
OUTSIDE_BASES = ["notebook", "sym1_binary"]


def _outside_basis(which):
    """(basis, whitening, model with that posterior, host rows of the wrapped frame)"""
    if which == "notebook":
        return RH.basis("bcc_mow"), SH.whitening("bcc_mow"), SH.posterior("bcc_mow"), SH.host_rows("bcc_mow", ORIGINAL)
    return (SH.sym1_basis(which), SH.sym1_whitening(which), SH.sym1_posterior(which), SH.sym1_rows(which, ORIGINAL))


@pytest.mark.parametrize("which", OUTSIDE_BASES)
@pytest.mark.parametrize("name", UNWRAPPED)
def test_an_atom_outside_its_cell_counts_as_its_image_inside(name, which):
    """Rows and grades describe the WRAPPED frame (include/uf3_hip.h).  On sym1_binary that includes the tie-break: the place of
    the wrapped image in the reference supercell decides the column, not the place of the atom as given."""
    inside, outside = RH.unwrapped_frames()[name]
    basis, w, model, host = _outside_basis(which)
    B_in, B_out = _rows(basis, [inside]), _rows(basis, [outside])
    scale = np.abs(B_in).max()
    errs = dict(outside_against_wrapped=float(np.abs(B_out - B_in).max() / scale), outside_against_host=float(np.abs(B_out - host).max() / scale))
    _report(f"{which} {name}: rows of the frame with atoms outside", **errs, bound=RTOL)
    assert max(errs.values()) <= RTOL, errs
    _, g = _check_grades(basis, [outside], w, f"{which} {name} outside")
    g_in, fm_in, fa_in = _grades(basis, [inside], w)
    g_out, fm_out, fa_out = _grades(basis, [outside], w)
    assert fa_out[0] == fa_in[0] and np.array_equal(g_out, g)
    assert np.all(np.abs(g_out - g_in) <= ls.leverage_bound(B_in, w, 1) + ls.leverage_bound(B_out, w, 1))
    # the Python surfaces
    fz = process.BasisFeaturizer(basis)
    rows_py, off = fz.site_rows([outside])
    assert np.array_equal(rows_py, B_out) and list(off) == [0, len(outside)]
    calc = calculator.UFCalculator(model, md_skin=0.0)
    got = calc.get_site_grades(outside)
    assert np.array_equal(got["grade"], g_out) and got["frame_max"] == fm_out[0] and got["frame_argmax"] == fa_in[0]
    # the site energies share the lists and the leg rule: the same U from either frame, and the rows' own
    U_in, U_out = (calc.site_terms([a], virials=False)[0][0] for a in (inside, outside))
    c = np.asarray(model.coefficients, dtype=float)
    errs = dict(U=RH.rel(U_out, U_in), rows_c=RH.rel(B_out @ c, U_out))
    _report(f"{which} {name}: site energies of the frame with atoms outside", **errs, bound=RTOL)
    assert max(errs.values()) <= RTOL, errs
    sites = pipeline.DeviceLeverage(model, fz).sites([inside, outside])
    assert np.array_equal(sites["grade"][len(inside):], g_out) and np.array_equal(sites["grade"][:len(inside)], g_in)
    assert sites["frame_argmax"][0] == sites["frame_argmax"][1] == fa_in[0]


# ========================================================================================== 8. grade samples inside MD, skewed cell
N_SAMPLES = SH.MD_STEPS // SH.MD_EVERY


def _dynamics(atoms, vel):
    dyn = MolecularDynamics(_calc(SH.MD_PAIR[0]), [atoms], SH.MD_DT, masses=SH.MD_MASS)
    dyn.set_velocities(vel)
    return dyn


@functools.lru_cache(maxsize=None)
def _md_blocks(label):
    """NVE from RH.velocities on one description of bcc_mow in blocks of MD_EVERY steps, one sample each: (grade [n], grade_atom
    [n], the states read back after each block)"""
    case = SH.MD_PAIR[0]
    grade, atom, states = [], [], []
    with _dynamics(RH.frame(case, label), RH.velocities(case, label)) as dyn:
        for s in range(N_SAMPLES):
            rec = dyn.run(SH.MD_EVERY, grade_every=SH.MD_EVERY)
            assert rec["grade"].shape == (1, 1) and rec["steps_done"] == SH.MD_EVERY and list(rec["grade_step"]) == [(s + 1) * SH.MD_EVERY]
            grade.append(float(rec["grade"][0, 0]))
            atom.append(int(rec["grade_atom"][0, 0]))
            states.append(dyn.get_atoms()[0])
    return np.array(grade), np.array(atom), states


def _sample_against_the_state(calc, basis, w, grade, atom, state, what):
    """tests/test_gpu_site_grade.py::test_md_samples_leave_the_trajectory_alone: the record is get_site_grades of ``state``
    within the bound of its rows, and the atom named holds the maximum within it"""
    want = calc.get_site_grades(state)
    b = ls.leverage_bound(_rows(basis, [state]), w, 1)
    assert abs(grade - want["frame_max"]) <= b.max(), (what, grade, want["frame_max"])
    assert want["grade"][atom] >= want["grade"].max() - 2 * b.max(), what
    top = np.sort(want["grade"])[-2:]
    if top[1] - top[0] > 2 * b.max():
        assert atom == want["frame_argmax"], (what, atom, want["frame_argmax"])
    return abs(grade - want["frame_max"]) / b.max(), b


def test_md_samples_on_a_skewed_reflected_cell_are_the_grades_of_the_state():
    case, label = SH.MD_PAIR
    calc, basis, w = _calc(case), RH.basis(case), SH.whitening(case)
    grade, atom, states = _md_blocks(label)
    worst = max(_sample_against_the_state(calc, basis, w, grade[s], atom[s], states[s], (label, s))[0] for s in range(N_SAMPLES))
    _report(f"{case} {label}: {N_SAMPLES} MD samples against get_site_grades of the state read back", error_over_bound=float(worst))
    # ... and one run of 40 steps gives the same samples (blocks = one run: tests/test_gpu_site_grade.py, here on this cell)
    with _dynamics(RH.frame(case, label), RH.velocities(case, label)) as dyn:
        rec = dyn.run(SH.MD_STEPS, grade_every=SH.MD_EVERY)
    assert np.array_equal(rec["grade"][:, 0], grade) and np.array_equal(rec["grade_atom"][:, 0], atom)


def test_md_samples_of_the_original_and_the_description_side_by_side():
    case, label = SH.MD_PAIR
    d = RH.description(case, label)
    basis, w = RH.basis(case), SH.whitening(case)
    g0, a0, s0 = _md_blocks(ORIGINAL)
    g1, a1, s1 = _md_blocks(label)
    worst, asserted = 0.0, 0
    for s in range(N_SAMPLES):
        b0 = ls.leverage_bound(_rows(basis, [s0[s]]), w, 1)[a0[s]]
        b1 = ls.leverage_bound(_rows(basis, [s1[s]]), w, 1)[a1[s]]
        tol = b0 + b1 + SPREAD_FACTOR * SH.MD_HOST_SPREAD[s] * g0[s]
        over = abs(g1[s] - g0[s]) / tol
        print(f"sample {s}: grade {g0[s]!r} / {g1[s]!r}, difference {abs(g1[s] - g0[s]):.2e}, bound {tol:.2e}")
        assert over <= 1.0, (s, g0[s], g1[s], tol)
        worst = max(worst, over)
        # the host reference of the original's state: where it grants room, both runs name the same atom
        host = ls.leverage_reference(SR.site_rows(RH.oracle_basis(case), wrapped(s0[s]), basis.n_feats), w, 1)
        if SH.room(host) >= SH.ARGMAX_ROOM:
            assert d.src[a1[s]] == a0[s] == int(np.argmax(host)), (s, a0[s], a1[s])
            asserted += 1
    _report(f"{case} original / {label}: MD samples side by side", difference_over_bound=float(worst), argmax_asserted=asserted)
    assert asserted == N_SAMPLES                       # (the host module found 4e-2 and more of room in every sample)


def test_md_samples_from_atoms_outside_the_cell_describe_the_wrapped_state():
    """The driver keeps positions unwrapped and its forces follow the reference's finite image range (another trajectory than
    the wrapped start's: tests/test_gpu_redescribed.py); the grade samples take nearest images and describe the wrapped state."""
    case = SH.MD_PAIR[0]
    calc, basis, w = _calc(case), RH.basis(case), SH.whitening(case)
    outside = RH.unwrapped_frames()["every_atom"][1]
    worst = 0.0
    with _dynamics(outside, RH.velocities(case, ORIGINAL)) as dyn:
        for s in range(N_SAMPLES):
            rec = dyn.run(SH.MD_EVERY, grade_every=SH.MD_EVERY)
            state = dyn.get_atoms()[0]
            assert np.abs(np.asarray(state.get_positions()) @ np.linalg.inv(np.asarray(state.get_cell(), float))).max() > 1.5
            over, _ = _sample_against_the_state(calc, basis, w, float(rec["grade"][0, 0]), int(rec["grade_atom"][0, 0]), wrapped(state),
                                                ("every_atom", s))
            worst = max(worst, over)
    _report("bcc_mow every_atom outside: MD samples against get_site_grades of the wrapped state", error_over_bound=float(worst))


def test_md_stops_on_the_same_sample_in_both_descriptions():
    case, label = SH.MD_PAIR
    maxima = _md_blocks(ORIGINAL)[0]
    rising = [s for s in range(N_SAMPLES - 1) if maxima[s + 1] > maxima[:s + 1].max()
              and abs(maxima[s + 1] - maxima[s]) >= SH.ARGMAX_ROOM * max(maxima[s], maxima[s + 1])]
    assert rising, maxima
    s = rising[0]
    stop = 0.5 * (maxima[s] + maxima[s + 1])
    assert maxima[:s + 1].max() < stop < maxima[s + 1]
    done = (s + 2) * SH.MD_EVERY
    for lab in (ORIGINAL, label):
        with _dynamics(RH.frame(case, lab), RH.velocities(case, lab)) as dyn:
            rec = dyn.run(SH.MD_STEPS, grade_every=SH.MD_EVERY, grade_stop=stop)
            assert rec["steps_done"] == done == dyn.step, (lab, rec["steps_done"], done)
        assert np.array_equal(rec["grade"][:, 0], _md_blocks(lab)[0][:s + 2]), lab
    print(f"grade_stop {stop!r} between samples {s} and {s + 1} of {maxima}: both descriptions stop after {done} steps")
