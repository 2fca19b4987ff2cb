"""Every device kernel that evaluates a spline, on distances that fall exactly on knots and on untrimmed leg ends
(tests/_on_knots.py): isolated pairs and triplets with one leg on a knot, or one and two units of 2^-42 A to either side of
it, for every knot of every sequence; commensurate crystals whose shells fall on knots and on r_max3; small frames for the NumPy
restatements.  tests/test_on_knots_host.py shows that on these frames every formulation of a distance gives the same double, so
the side of a knot a kernel puts it on is the kernel's own doing, and that with an untrimmed leading edge the wrong side moves a
column of the energy row by order one.

The convention held: knot interval (t_i, t_i+1], leg ends strict -- the reference's rows.

Every bound is the one the existing test of the same kernel uses; its source is named next to it.  The reference is always the
oracle or a NumPy restatement, never a second device route."""
import ctypes as C
import functools

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import _lib
from uf3_amd.forcefield import calculator, harmonic
from uf3_amd.regression import least_squares as ls
from uf3_amd.representation import process
import _flux_ref as FR
import _harmonic_ref as HR
import _on_knots as K
import _site_rows_ref as SR
from _util import dbg, rel_err, worst_elementwise  # noqa: F401  (dbg: the fixture)
from test_gpu_mc import _check_deltas
from test_gpu_virial import _MD_ROUTES

pytestmark = pytest.mark.gpu
TOL = 1e-9                   # tests/test_gpu_parity.py::_check_against_oracle, tests/test_gpu_virial.py, tests/test_gpu_mc.py
FLUX_RTOL = 1e-10            # tests/test_gpu_flux.py::test_device_against_restatement
ROWS_RTOL = 1e-10            # tests/test_gpu_site_grade.py::test_rows_against_the_host_rows
HESSIAN_RTOL = 1e-10         # tests/test_gpu_harmonic.py::test_device_against_restatement
MASS = {42: 95.95, 74: 183.84}

# featurizer_modes bits (include/uf3_hip.h).  Bit 7 is the (1, 2)-tile matrix-core mode; grouped windows are chosen inside it, for
# 3 x 3 x 6..9 windows (uf3_basis_create), which is grid_notebook_lead3's shape: the mask cannot say "grouped", the shape does.
GENERIC, MFMA_TWO_TILE, MFMA_OTHER, FEAT3 = 0x3e, 1 << 7, (1 << 6) | (1 << 8) | (1 << 9), 1 << 12

# Which k_eval instances a basis qualifies for follows from the basis alone (uf3_basis_create: eval_tab_ok, eval_cw_ok; uf3_eval:
# tab, cw, win).  TAB: one set of 3-body legs for all trios and at most 24 intervals on leg n -- the five one-trio bases, not
# grid_binary.  The CW / WIN window table: centre-leg windows of 3 kept bins -- grid_notebook_lead3 alone (leading trim 0 keeps 6,
# trailing trim 2 keeps 4).
TAB_BASES = [name for name in K.BASES if name != "grid_binary"]
CW_BASES = ["grid_notebook_lead3"]


def _instance(name, md, gather, no_tab=False, no_cw=False, cap=16):
    """the (tab, cw, win) flags uf3_eval must report: TAB on the two-pass routes of a qualifying basis, CW for its MD steps with
    lists of at most 16 entries, WIN where the window table exists and CW does not serve"""
    tab = int(name in TAB_BASES and not gather and not no_tab)
    cw = int(tab and md and name in CW_BASES and cap <= 16 and not no_cw)
    win = int(tab and not cw and name in CW_BASES and not no_cw)
    return {"tab": tab, "cw": cw, "win": win}


@functools.lru_cache(maxsize=None)
def _ob(name):
    return O.OracleBasis(K.basis(name))


@functools.lru_cache(maxsize=None)
def _model(name):
    model = ls.WeightedLinearModel(K.basis(name))
    model.coefficients = K.coefficients(K.basis(name))
    return model


def _calc(name, skin=0.0):
    return calculator.UFCalculator(_model(name), md_skin=skin)


def _coeff(name):
    return np.asarray(_model(name).coefficients, dtype=float)


def _frames(name):
    """the probe frames, then the crystals"""
    return K.probe_frames(name) + K.crystals(name)


def _vanishing(name, k):
    """frame k of _frames is a perfect one-species crystal: every force and force row is a sum that cancels to zero"""
    n_probe = len(K.probe_frames(name))
    return k >= n_probe and K.forces_vanish(name, k - n_probe)


@pytest.fixture(scope="module", autouse=True)
def _references_leave_with_the_module():
    yield
    for cached in (_oracle_rows, _frame_reference, _small_reference, _hessian_reference):
        cached.cache_clear()


# ------------------------------------------------------------------------------------------------ the featurizer
def test_the_bases_reach_every_featurizer_family():
    """k_featurize3, a matrix-core mode with grouped windows, a dense or banded matrix-core mode and the generic kernels"""
    modes = {}
    for name in K.BASES:
        b = K.basis(name)
        modes[name] = process.BasisFeaturizer(b)._dev()[1].featurizer_modes
        print(f"{name}: F = {b.n_feats}, featurizer modes {modes[name]:#06x}")
    assert modes["grid_notebook_lead3"] & MFMA_TWO_TILE and modes["grid_notebook_lead3"] & FEAT3     # 3 x 3 x 9 windows: grouped
    assert [int(n) - 4 - 6 for n in map(len, K.basis("grid_notebook_lead3").knots_map[("W", "W", "W")])] == [3, 3, 9]
    assert any(m & MFMA_OTHER for m in modes.values())
    assert any(m & GENERIC for m in modes.values())
    assert sum(bool(m & FEAT3) for m in modes.values()) >= 2


@functools.lru_cache(maxsize=None)
def _oracle_rows(name, k):
    """(x_e, x_f, [dE/dstrain of four coefficient vectors]) of frame k: computed once, shared, never changed"""
    atoms = _frames(name)[k]
    ref = O.featurize(_ob(name), atoms)
    vir = np.array([O.evaluate(_ob(name), atoms, K.coefficients(K.basis(name), 100 + q), forces=False, virial=True)[2] for q in range(4)])
    for a in (ref["xe"], ref["xf"], vir):
        a.setflags(write=False)
    return ref["xe"], ref["xf"], vir


def _check_rows(name, k, x_e, x_f, x_v, label):
    """tests/test_gpu_parity.py::_check_against_oracle (max-norm and entry by entry, 1e-9) and tests/test_gpu_virial_rows.py::
    _against_oracle_through_coefficients (worst_elementwise, rtol 1e-9, floor 1e-11).  On a perfect one-species crystal every
    force row is zero up to rounding and has no magnitude of its own to be relative to: the max-norm bound alone."""
    r_e, r_f, r_v = _oracle_rows(name, k)
    b = K.basis(name)
    errs = [rel_err(x_e, r_e), worst_elementwise(x_e, r_e, rtol=TOL), rel_err(x_f, r_f),
            0.0 if _vanishing(name, k) else worst_elementwise(x_f, r_f, rtol=TOL),
            max(worst_elementwise(x_v @ K.coefficients(b, 100 + q), r_v[q], rtol=1e-9, floor=1e-11) for q in range(4))]
    print(f"{label} frame {k} ({x_f.shape[0]} atoms): x_e {errs[0]:.2e} (bound {TOL:.0e}) / {errs[1]:.2e} (1), "
          f"x_f {errs[2]:.2e} / {errs[3]:.2e}, x_v @ c {errs[4]:.2e} (1)")
    assert errs[0] < TOL and errs[1] <= 1.0 and errs[2] < TOL and errs[3] <= 1.0 and errs[4] <= 1.0, (label, k, errs)


FEATURIZER_ROUTES = {"default": {}, "no_feat3": {"UF3_NO_FEAT3": "1"}, "generic": {"UF3_NO_FEAT3": "1", "UF3_NO_MFMA_FEAT": "1"}}


@pytest.mark.parametrize("route", list(FEATURIZER_ROUTES))
@pytest.mark.parametrize("name", K.BASES)
def test_featurizer_rows(name, route, monkeypatch):
    """Energy, force and virial rows of every probe frame and crystal, as one ragged batch and frame by frame, through the
    default launches, without k_featurize3 and on the generic kernels (the switches are read when the device tables are made)."""
    b = K.basis(name)
    for key, val in FEATURIZER_ROUTES[route].items():
        monkeypatch.setenv(key, val)
    _lib.drop_device_basis(b)
    try:
        fz = process.BasisFeaturizer(b)
        modes = fz._dev()[1].featurizer_modes
        print(f"{name} {route}: featurizer modes {modes:#06x}")
        if route != "default":
            assert not modes & FEAT3
        if route == "generic":
            assert not modes & (MFMA_TWO_TILE | MFMA_OTHER) and modes & GENERIC
        frames = list(_frames(name))
        x_e, x_f, off = fz.featurize_frames(frames)
        x_v = fz.featurize_virials(frames)
        for k in range(len(frames)):
            _check_rows(name, k, x_e[k], x_f[off[k]:off[k + 1]], x_v[k], f"{name} {route} batch")
        for k, atoms in enumerate(frames):
            e1, f1, _ = fz.featurize_frames([atoms])
            _check_rows(name, k, e1[0], f1, fz.featurize_virials([atoms])[0], f"{name} {route} alone")
    finally:
        _lib.drop_device_basis(b)                  # (tables made under a switch do not outlive the test)


# ------------------------------------------------------------------------------------------------ the evaluator
@functools.lru_cache(maxsize=None)
def _frame_reference(name, k):
    out = O.evaluate(_ob(name), _frames(name)[k], _coeff(name), virial=True)
    for a in out[1:]:
        a.setflags(write=False)
    return out


def _check_frame(e, f, v, ref, label, vanishing=False):
    """tests/test_gpu_virial.py::_check_frame.  Forces that vanish by symmetry (a perfect one-species crystal) have no magnitude
    of their own: tests/test_gpu_parity.py's max-norm bound on evaluator forces, rel_err < 1e-9, in place of the entry-wise one."""
    e_o, f_o, v_o = ref
    err_f = None if f is None else (rel_err(f, f_o) / TOL if vanishing else worst_elementwise(f, f_o, TOL))
    err_v = worst_elementwise(v, v_o, rtol=1e-9, floor=1e-11)
    print(f"{label}: |dE| / max(1, |E|) = {abs(e - e_o) / max(1.0, abs(e_o)):.2e} (bound {TOL:.0e}), F "
          f"{'-' if err_f is None else format(err_f, '.2e')}, dE/dstrain {err_v:.2e} (bound 1)")
    assert abs(e - e_o) <= TOL * max(1.0, abs(e_o)), (label, e, e_o)
    if f is not None:
        assert err_f <= 1.0, label
    assert err_v <= 1.0, (label, v, v_o)


@pytest.mark.parametrize("name", K.BASES)
def test_evaluator_plain_and_gather_routes(name, dbg, monkeypatch):
    """md_skin = 0: the ragged batch of every probe frame and crystal through the centre pass + collection pass, through the
    gather instance (UF3_EVAL_GATHER, and without forces), and every frame alone.  Bounds: tests/test_gpu_virial.py::
    test_plain_route_on_a_ragged_batch_host_and_device_entries.  The centre pass runs the TAB instance on the bases that qualify
    (reading the window table, WIN, where there is one), the gather role never does: asserted from the launch report."""
    dbg.basis(K.basis(name))
    calc = _calc(name)
    frames = list(_frames(name))
    for _ in range(2):
        calc.evaluate_frames(frames, virial=True)                     # (list capacity tuned)
    dbg.launches()
    for label, env, forces in (("plain", {}, True), ("gather", {"UF3_EVAL_GATHER": "1"}, True), ("forces=False", {}, False)):
        for key, val in env.items():
            monkeypatch.setenv(key, val)
        e, f, off, v = calc.evaluate_frames(frames, forces=forces, virial=True)
        for key in env:
            monkeypatch.delenv(key)
        said = dbg.launches()
        gather = int(label != "plain")
        assert said and all(s["vir"] == 1 and s["md"] == 0 and s["gather"] == gather for s in said), said
        want = _instance(name, md=False, gather=bool(gather))
        assert all(s[key] == val for s in said for key, val in want.items()), (name, label, want, said)
        assert (f is None) == (not forces)
        for k in range(len(frames)):
            _check_frame(e[k], None if f is None else f[off[k]:off[k + 1]], v[k], _frame_reference(name, k),
                         f"{name} {label} frame {k}", _vanishing(name, k))
    for k, atoms in enumerate(frames):
        e, f, _, v = calc.evaluate_frames([atoms], virial=True)
        _check_frame(e[0], f, v[0], _frame_reference(name, k), f"{name} frame {k} alone", _vanishing(name, k))


@pytest.mark.parametrize("route", list(_MD_ROUTES))
@pytest.mark.parametrize("name", K.BASES)
def test_evaluator_md_routes(name, route, dbg, monkeypatch):
    """The MD route (skin 0.5) and every switch that takes a step elsewhere: the first probe frame and the crystals as one batch,
    then one frame of probes walked from q = -1 over q = 0 to q = +1 -- two displacements of 2^-42 A that carry every probed
    distance across its knot, served from the lists of the first step.  Every step against the oracle.  Bounds and instance flags:
    tests/test_gpu_virial.py::test_md_route_instances_on_every_step_of_a_walk.  Every entry of _MD_ROUTES is asserted on every
    step, and with it the TAB, CW and WIN flags the basis qualifies for (``_instance``; where _MD_ROUTES names one of them the
    two agree on the qualifying bases, and grid_binary, which has no TAB instance, reports 0).  So the LDS-table instances are
    known to have handled pure probe frames on every basis with leading trim 0 but grid_binary, the CW instance (lists of at
    most 16 entries) and the WIN instance those of grid_notebook_lead3.  On the routes that stay on the MD route the two walk
    steps must come from the first step's lists: at most one build.  The routes a switch takes off the MD route (gather,
    separate_n3, no_md) keep no lists, and nothing is asserted of the build count there."""
    env, want = _MD_ROUTES[route]
    md, gather = bool(want.get("md", 0)), bool(want.get("gather", 0))

    def wanted(cap):
        own = _instance(name, md, gather, no_tab=route == "no_tab", no_cw=route in ("no_cw", "no_tab"), cap=cap)
        if name in TAB_BASES:
            assert all(own[key] == val for key, val in want.items() if key in own), (route, want, own)
        return {**want, **own}
    dbg.basis(K.basis(name))
    n_probe = len(K.probe_frames(name))
    ks = [0] + list(range(n_probe, len(_frames(name))))
    batch = [_frames(name)[k] for k in ks]
    walk = K.walk_frames(name)
    plain = _calc(name)
    for _ in range(2):
        plain.evaluate_frames(batch, virial=True)                     # (capacity tuned: the MD route starts from a tuned context)
        plain.evaluate_frames([walk[0]], virial=True)
    for key, val in env.items():
        monkeypatch.setenv(key, val)
    calc = _calc(name, skin=0.5)
    dbg.launches()
    e, f, off, v = calc.evaluate_frames(batch, virial=True)
    said = dbg.launches()
    print(f"{name} {route}: {said[-1] if said else said}")
    assert said and said[-1]["vir"] == 1, (route, said)
    assert all(said[-1][key] == val for key, val in wanted(said[-1]["cap"]).items()), (route, wanted(said[-1]["cap"]), said)
    if name in CW_BASES and route in ("default", "no_cap16"):
        assert said[-1]["cw"] == 1 and said[-1]["cap"] <= 16, said           # (short lists: the CW instances, both cap16 settings)
    for q, k in enumerate(ks):
        _check_frame(e[q], f[off[q]:off[q + 1]], v[q], _frame_reference(name, k), f"{name} {route} batch frame {k}", _vanishing(name, k))
    calc = _calc(name, skin=0.5)
    ctx = _lib.get_context(None)
    before = ctx.md_stats()
    for q, atoms in zip((-1, 0, 1), walk):
        e, f, _, v = calc.evaluate_frames([atoms], virial=True)
        said = dbg.launches()
        assert said and said[-1]["vir"] == 1, (route, q, said)
        assert all(said[-1][key] == val for key, val in wanted(said[-1]["cap"]).items()), (route, q, wanted(said[-1]["cap"]), said)
        if name in CW_BASES and route in ("default", "no_cap16"):
            assert said[-1]["cw"] == 1 and said[-1]["cap"] <= 16, said
        _check_frame(e[0], f, v[0], O.evaluate(_ob(name), atoms, _coeff(name), virial=True), f"{name} {route} walk q = {q:+d}")
    after = ctx.md_stats()
    print(f"{name} {route}: md_stats before {before}, after {after}")
    if md:
        assert after["steps"] - before["steps"] >= 2 and after["builds"] - before["builds"] <= 1, (before, after)  # (kept lists)


# ------------------------------------------------------------------------------------------------ the small frames
@functools.lru_cache(maxsize=None)
def _small_reference(name, which):
    """what the NumPy restatements say of a small frame: computed once, shared, never changed"""
    ob, a, c = _ob(name), K.small_frames(name)[which], _coeff(name)
    out = dict(eval=O.evaluate(ob, a, c, virial=True), site=FR.site_terms(ob, a, c), xe=O.featurize(ob, a, forces=False)["xe"])
    for v in (out["eval"][1], out["eval"][2], out["site"][0], out["site"][1], out["xe"]):
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _hessian_reference(name, which):
    out = HR.hessian(_ob(name), K.small_frames(name)[which], _coeff(name))
    for a in out:
        a.setflags(write=False)
    return out


@pytest.mark.parametrize("name,which", K.SMALL_CASES)
def test_hessian(name, which):
    """uf3_hessian with the mixed and Born terms on the small probe frame, the 16-atom crystal and (one species) that crystal
    with a vacancy.  Bound: tests/test_gpu_harmonic.py::test_device_against_restatement (1e-10 of the largest entry).  On the
    perfect one-species crystal the mixed term d2E / dx dt vanishes by symmetry, a sum of terms that cancel: there the largest
    entry is taken from the same lattice with the vacancy, where they do not."""
    calc = _calc(name)
    atoms = K.small_frames(name)[which]
    ref_H, ref_L, ref_B = _hessian_reference(name, which)
    H, L, B, _ = harmonic.hessian(calc, atoms, strain=True)
    size_L = np.abs(_hessian_reference(name, 2)[1]).max() if which == 1 and K.forces_vanish(name, 0) else np.abs(ref_L).max()
    errs = [np.abs(H - ref_H).max() / np.abs(ref_H).max(), np.abs(L - ref_L).max() / size_L, np.abs(B - ref_B).max() / np.abs(ref_B).max()]
    print(f"{name} frame {which}: H {errs[0]:.2e}, mixed {errs[1]:.2e}, Born {errs[2]:.2e} of the largest entry (bound {HESSIAN_RTOL:.0e})")
    assert np.array_equal(harmonic.hessian(calc, atoms), H)
    assert max(errs) <= HESSIAN_RTOL, errs


def _vel(atoms, seed):
    return np.random.default_rng(seed).normal(0, 0.01, (len(atoms), 3))


def _masses(atoms):
    return np.array([MASS[int(q)] for q in atoms.get_atomic_numbers()])


@pytest.mark.parametrize("name", K.BASES)
def test_site_terms_and_heat_flux(name):
    """The small frames in one batch: U, W, J_conv and J_pot.  Bounds: tests/test_gpu_flux.py::test_device_against_restatement
    (1e-10 of each quantity's largest magnitude; J_pot: of the sum of its terms' absolute values)."""
    calc = _calc(name)
    frames = list(K.small_frames(name))
    vel = [_vel(a, 50 + k) for k, a in enumerate(frames)]
    masses = [_masses(a) for a in frames]
    Us, Ws = calc.site_terms(frames)
    flux = calc.heat_flux(frames, np.concatenate(vel), np.concatenate(masses))
    for k, a in enumerate(frames):
        rU, rW = _small_reference(name, k)["site"]
        rJc, rJp, scale = FR.heat_flux(_ob(name), a, vel[k], masses[k], _coeff(name), with_scale=True)
        errs = (np.abs(Us[k] - rU).max() / np.abs(rU).max(), np.abs(Ws[k] - rW).max() / np.abs(rW).max(),
                np.abs(flux[k][0] - rJc).max() / np.abs(rJc).max(), (np.abs(flux[k][1] - rJp) / scale).max())
        print(f"{name} frame {k}: U {errs[0]:.2e}, W {errs[1]:.2e}, J_conv {errs[2]:.2e}, J_pot {errs[3]:.2e} (bound {FLUX_RTOL:.0e})")
        assert scale.min() > 0 and max(errs) <= FLUX_RTOL, (k, errs)


def _site_rows(basis, frames):
    """tests/test_gpu_site_grade.py::_rows"""
    ctx = _lib.get_context(None)
    db = _lib.device_basis(basis, ctx)
    batch = _lib.FrameBatch(list(frames))
    rows = np.empty((batch.n_atoms, db.n_feat))
    ctx.check(ctx.lib.uf3_site_rows(db.handle, C.byref(batch.struct), _lib._p(batch.pos), _lib._p(batch.z), _lib._p(rows), db.n_feat))
    return rows


def _site_grades(basis, frames, w):
    """tests/test_gpu_site_grade.py::_grades"""
    ctx = _lib.get_context(None)
    db = _lib.device_basis(basis, ctx)
    batch = _lib.FrameBatch(list(frames))
    w = np.ascontiguousarray(w, dtype=np.float64)
    g, fm, fa = np.empty(batch.n_atoms), np.empty(batch.n_frames), np.empty(batch.n_frames, dtype=np.int32)
    ctx.check(ctx.lib.uf3_site_grade(db.handle, C.byref(batch.struct), _lib._p(batch.pos), _lib._p(batch.z), _lib._p(w), _lib._p(g),
                                     _lib._p(fm), _lib._p(fa)))
    return g, fm, fa


@pytest.mark.parametrize("name", K.BASES)
def test_site_rows_and_grades(name):
    """uf3_site_rows against the host rows on both small frames (tests/test_gpu_site_grade.py::test_rows_against_the_host_rows:
    1e-10 of the largest |B|); their sum against the oracle's energy row on the columns the featurizer fills (it leaves the
    frozen pair columns at zero: ::test_rows_against_site_energies_and_the_energy_row); uf3_site_grade against
    ls.leverage_reference of the device's rows, just held to the host's, within ls.leverage_bound (::_check_grades)."""
    b = K.basis(name)
    frames = list(K.small_frames(name))
    rows = _site_rows(b, frames)
    off = np.concatenate([[0], np.cumsum([len(a) for a in frames])])
    live = np.setdiff1d(np.arange(b.n_feats), np.asarray(b.col_idx, dtype=int))
    for k, a in enumerate(frames):
        B = SR.site_rows(_ob(name), a, b.n_feats)
        got = rows[off[k]:off[k + 1]]
        err = np.abs(got - B).max() / np.abs(B).max()
        x_e = _small_reference(name, k)["xe"]
        err_e = np.abs(got.sum(axis=0) - x_e)[live].max() / np.abs(x_e).max()
        print(f"{name} frame {k}: rows {err:.2e}, their sum against the oracle's energy row {err_e:.2e} (bound {ROWS_RTOL:.0e})")
        assert err <= ROWS_RTOL and err_e <= ROWS_RTOL
    w = SR.seeded_model(b).whitening()
    g, fm, fa = _site_grades(b, frames, w)
    ref, bound = ls.leverage_reference(rows, w, 1), ls.leverage_bound(rows, w, 1)
    print(f"{name}: max grade {ref.max():.3e}, worst error / bound {(np.abs(g - ref) / bound).max():.2e}")
    assert np.all(np.abs(g - ref) <= bound)
    for k in range(len(frames)):
        seg = g[off[k]:off[k + 1]]
        assert fm[k] == seg.max() and fa[k] == int(np.flatnonzero(seg == seg.max())[0])


@pytest.mark.parametrize("which", [0, 1])
def test_mc_delta_energy(which):
    """grid_binary: every swap of unlike atoms and every transmutation of a small frame moves triplets across the trios' own
    leg ends.  tests/test_gpu_mc.py::_check_deltas against the oracle, 1e-9 max(1, |E|)."""
    name = "grid_binary"
    calc = _calc(name)
    ob, coeff = _ob(name), _coeff(name)
    _check_deltas(calc, K.small_frames(name)[which], lambda frames: np.array([O.evaluate(ob, a, coeff, forces=False)[0] for a in frames]))


@pytest.mark.parametrize("name", K.BASES)
def test_kernel_families_agree_on_the_energy(name):
    """The evaluator's energy (r_jk from norm3_leg), the sum of the site energies (norm3_rn) and the featurizer's energy row
    times the coefficients, each against the oracle within its own bound (tests/test_gpu_virial.py: 1e-9 max(1, |E|);
    tests/test_gpu_uneven_legs.py::test_site_terms_and_heat_flux for the sum of U), and so against each other within their sum:
    one family taking an r_jk = t0 probe for inside and another for outside would be off by order one."""
    calc = _calc(name)
    frames = list(K.small_frames(name))
    e = calc.evaluate_frames(frames, forces=False)[0]
    Us = calc.site_terms(frames, virials=False)[0]
    x_e = process.BasisFeaturizer(K.basis(name)).featurize_frames(frames, forces=False)[0]
    for k in range(len(frames)):
        e_o = _small_reference(name, k)["eval"][0]
        got = (float(e[k]), float(Us[k].sum()), float(x_e[k] @ _coeff(name)))
        tol = TOL * max(1.0, abs(e_o))
        print(f"{name} frame {k}: evaluator, sum of U, x_e @ c = {got}, oracle {e_o} (tol {tol:.1e})")
        assert all(abs(x - e_o) <= tol for x in got), (got, e_o)
        assert max(got) - min(got) <= 2 * tol
