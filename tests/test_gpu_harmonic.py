"""The device Hessian (uf3_hessian, uf3_amd.forcefield.harmonic) against the NumPy restatement, finite differences of the
device forces and the oracle, its exact identities, bitwise repeatability, and the phonon / elastic drivers on bcc W."""
import os

import numpy as np
import pytest

from oracle import oracle as O
from uf3_amd import synthetic
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import calculator, harmonic
from uf3_amd.regression import least_squares as ls
import _harmonic_ref as HR
from _util import GOLDEN, basis_from_meta, equivalence_cases, load_case, wrapped

pytestmark = pytest.mark.gpu

A0_W = 3.17352          # model_unary.json: zero virial trace (oracle, CPU); the tests find their own by bisection
W_MASS = {"W": 183.84}


def _unary_model():
    return ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json"))


def _seeded_model(basis, seed):
    model = ls.WeightedLinearModel(basis)
    coeff = np.random.default_rng(seed).normal(0, 0.05, basis.n_feats)
    coeff[basis.col_idx] = 0.0
    model.coefficients = coeff
    return model


def _mow_model():
    return _seeded_model(synthetic.notebook_basis(["Mo", "W"]), 31)


def _case_model(name, seed):
    _, meta, atoms = load_case(name)
    return (lambda: _seeded_model(basis_from_meta(meta), seed)), atoms


def _calc(model):
    return calculator.UFCalculator(model, md_skin=0.0)


def _bcc(a, reps, z=74):
    base = np.array([[0, 0, 0], [0.5, 0.5, 0.5]])
    grid = np.array(list(np.ndindex(*reps)), dtype=float)
    pos = ((grid[:, None, :] + base[None]) * a).reshape(-1, 3)
    return Atoms(numbers=np.full(len(pos), z), positions=pos, cell=np.diag(np.array(reps, dtype=float) * a), pbc=True)


def _cases():
    w = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=3)
    mow = synthetic.lattice_frame("bcc", (2, 2, 2), 3.2, [42, 74], seed=5)
    cl = synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=7)
    cl = Atoms(numbers=cl.get_atomic_numbers(), positions=cl.get_positions(), cell=np.zeros((3, 3)), pbc=False)
    sl = synthetic.lattice_frame("bcc", (2, 2, 2), 3.2, [42, 74], seed=9)
    sl = Atoms(numbers=sl.get_atomic_numbers(), positions=sl.get_positions(), cell=sl.get_cell(), pbc=[True, True, False])
    small = synthetic.lattice_frame("bcc", (1, 1, 1), 3.2, [42, 74], seed=11)      # cell below the cut-off: self-images
    s4_model, s4 = _case_model("case_bcc24_s4", 41)            # four species
    nexe_model, nexe = _case_model("case_nexe32", 37)            # 2-body only
    ghost = equivalence_cases()["slab_ghost_terms"][2][0].atoms  # skewed slab, plane spacing 3.0 A along a
    return [("w16", _unary_model, w), ("mow16", _mow_model, mow), ("w_cluster", _unary_model, cl), ("mow_slab", _mow_model, sl),
            ("mow_tiny", _mow_model, small), ("bcc24_s4", s4_model, s4), ("nexe32_2body", nexe_model, nexe),
            ("slab_ghost_terms", _mow_model, ghost)]


@pytest.mark.parametrize("label,model,atoms", _cases(), ids=[c[0] for c in _cases()])
def test_device_against_restatement(label, model, atoms):
    m = model()
    calc = _calc(m)
    ref_H, ref_L, ref_B = HR.hessian(O.OracleBasis(m.bspline_config), atoms, np.asarray(m.coefficients, dtype=float))
    H = harmonic.hessian(calc, atoms)
    assert np.abs(H - ref_H).max() <= 1e-10 * np.abs(ref_H).max()
    if np.all(atoms.get_pbc()):
        H2, L, B, vir = harmonic.hessian(calc, atoms, strain=True)
        assert np.array_equal(H2, H)
        assert np.abs(L - ref_L).max() <= 1e-10 * np.abs(ref_L).max()
        assert np.abs(B - ref_B).max() <= 1e-10 * np.abs(ref_B).max()


def test_device_against_device_force_differences():
    calc = _calc(_seeded_model(synthetic.notebook_basis(["Nb", "Mo", "W"]), 43))
    atoms = synthetic.lattice_frame("bcc", (3, 3, 3), 3.2, [41, 42, 74], seed=13)       # 54 atoms, ternary
    assert len(set(atoms.get_atomic_numbers().tolist())) == 3
    pos = np.asarray(atoms.get_positions(), dtype=float)
    n = len(pos)
    H = harmonic.hessian(calc, atoms)
    h = 1e-5
    frames = []
    for k in range(3 * n):
        for sgn in (1, -1):
            p = pos.copy()
            p[k // 3, k % 3] += sgn * h
            frames.append(Atoms(numbers=atoms.get_atomic_numbers(), positions=p, cell=atoms.get_cell(), pbc=True))
    f = calc.evaluate_frames(frames)[1].reshape(3 * n, 2, 3 * n)
    Hfd = -(f[:, 0] - f[:, 1]).T / (2 * h)
    assert np.abs(H - Hfd).max() <= 1e-6 * np.abs(H).max()


def test_identities_slabs_and_repeatability():
    calc = _calc(_mow_model())
    atoms = synthetic.lattice_frame("bcc", (10, 10, 10), 3.2, [42, 74], seed=17)
    n = len(atoms.get_atomic_numbers())
    e0, f0, _, v0 = calc.evaluate_frames([atoms], virial=True)
    H = harmonic.hessian(calc, atoms)
    scale = np.abs(H).max()
    sums = H.reshape(3 * n, n, 3).sum(axis=1)
    assert np.abs(sums).max() <= 1e-11 * scale
    assert np.abs(H - H.T).max() <= 1e-12 * scale
    assert np.array_equal(harmonic.hessian(calc, atoms), H)
    parts = [harmonic.hessian(calc, atoms, rows=(lo, min(lo + 700, n))) for lo in range(0, n, 700)]
    assert np.array_equal(np.concatenate(parts), H)
    Hw = harmonic.hessian(calc, wrapped(atoms))
    assert np.abs(Hw - H).max() <= 1e-12 * scale
    e1, f1, _, v1 = calc.evaluate_frames([atoms], virial=True)
    assert np.array_equal(e0, e1) and np.array_equal(f0, f1) and np.array_equal(v0, v1)
    skin = calculator.UFCalculator(_mow_model(), md_skin=0.5)
    a = skin.evaluate_frames([atoms], virial=True)
    skin.evaluate_frames([atoms], virial=True)
    harmonic.hessian(skin, atoms)
    b = skin.evaluate_frames([atoms], virial=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def _virial_trace(calc, a):
    return float(np.sum(calc.evaluate_frames([_bcc(a, (1, 1, 1))], virial=True)[3][0][:3]))


@pytest.fixture(scope="module")
def a0():
    """Lattice constant of bcc W under model_unary.json: bisection on the virial trace of the conventional cell."""
    calc = _calc(_unary_model())
    lo, hi = 3.10, 3.25
    f_lo, f_hi = _virial_trace(calc, lo), _virial_trace(calc, hi)
    assert f_lo * f_hi < 0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        f = _virial_trace(calc, mid)
        if (f < 0) == (f_lo < 0):
            lo, f_lo = mid, f
        else:
            hi = mid
    a = 0.5 * (lo + hi)
    assert abs(a - A0_W) < 1e-4
    return a


def _strained(atoms, eps):
    return Atoms(numbers=atoms.get_atomic_numbers(), positions=np.asarray(atoms.get_positions()) @ eps.T,
                 cell=np.asarray(atoms.get_cell()) @ eps.T, pbc=True)


def _eps(pairs):
    """I + eps for [(voigt component, t), ...] (engineering shear: eps_ab = eps_ba = t / 2)."""
    eps = np.eye(3)
    for k, t in pairs:
        a, b = harmonic._VOIGT[k]
        if a == b:
            eps[a, a] += t
        else:
            eps[a, b] += 0.5 * t
            eps[b, a] += 0.5 * t
    return eps


def _quiet_elastic(calc, atoms, relaxed=True):
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        return harmonic.elastic_tensor(calc, atoms, relaxed=relaxed)


def test_elastic_constants_bcc_w(a0):
    m = _unary_model()
    calc = _calc(m)
    atoms = _bcc(a0, (1, 1, 1))
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", RuntimeWarning)
        got = calc.get_elastic_constants(atoms)
    ob = O.OracleBasis(m.bspline_config)
    coeff = np.asarray(m.coefficients, dtype=float)
    vol = a0 ** 3
    d = 1e-4

    def second(u, v):
        out = 0.0
        for su, sv, w in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1)):
            out += w * O.evaluate(ob, _strained(atoms, _eps([(u, su * d), (v, sv * d)])), coeff)[0]
        return out / (4 * d * d) / vol * harmonic.EV_PER_A3_GPA

    c11, c12, c44 = second(0, 0), second(0, 1), second(5, 5)
    want = [c11, c12, c44, (c11 + 2 * c12) / 3]
    assert np.allclose(got, want, rtol=1e-4, atol=0), (got, want)


def _relax(calc, atoms, fmax=1e-9, steps=40):
    """Newton steps on the device Hessian (rigid translations left alone) to max |F| < fmax; (frame, energy)."""
    pos = np.asarray(atoms.get_positions(), dtype=float).copy()
    for _ in range(steps):
        a = Atoms(numbers=atoms.get_atomic_numbers(), positions=pos, cell=atoms.get_cell(), pbc=True)
        e, f, _ = calc.evaluate_frames([a])
        if np.abs(f).max() < fmax:
            return a, float(e[0])
        H = harmonic.hessian(calc, a)
        pos = pos + np.linalg.lstsq(H, f.ravel(), rcond=1e-10)[0].reshape(-1, 3)
    raise AssertionError(f"Newton relaxation did not reach max|F| < {fmax}: {np.abs(f).max()}")


def test_relaxed_ion_elastic_constants_with_a_vacancy(a0):
    calc = _calc(_unary_model())
    perfect = _bcc(a0, (3, 3, 3))
    keep = np.arange(1, len(perfect.get_atomic_numbers()))
    start = Atoms(numbers=perfect.get_atomic_numbers()[keep], positions=np.asarray(perfect.get_positions())[keep],
                  cell=perfect.get_cell(), pbc=True)
    ref, e0 = _relax(calc, start)
    assert np.abs(np.asarray(ref.get_positions()) - np.asarray(start.get_positions())).max() > 1e-3     # the ions did move
    res = _quiet_elastic(calc, ref)
    C, Cc = res["C"], res["C_clamped"]
    assert np.abs(C - Cc).max() > 2e-4 * np.abs(C).max()          # relaxation matters beyond the tolerance below
    vol = abs(np.linalg.det(np.asarray(ref.get_cell())))
    d = 1e-3

    def e_rel(pairs):
        return _relax(calc, _strained(ref, _eps(pairs)))[1]

    def diag(u):
        f = {k: e_rel([(u, k * d)]) for k in (-2, -1, 1, 2)}
        return (-f[2] + 16 * f[1] - 30 * e0 + 16 * f[-1] - f[-2]) / (12 * d * d) / vol * harmonic.EV_PER_A3_GPA

    def mixed(u, v):
        def s(h):
            return sum(w * e_rel([(u, su * h), (v, sv * h)])
                       for su, sv, w in ((1, 1, 1), (1, -1, -1), (-1, 1, -1), (-1, -1, 1))) / (4 * h * h)
        return (4 * s(d) - s(2 * d)) / 3 / vol * harmonic.EV_PER_A3_GPA

    scale = np.abs(C).max()
    for (u, v), want in (((0, 0), diag(0)), ((3, 3), diag(3)), ((0, 1), mixed(0, 1))):
        assert abs(C[u, v] - want) <= 1e-4 * scale, ((u, v), C[u, v], want, Cc[u, v])
    assert np.all(np.linalg.eigvalsh(Cc - C) >= -1e-9 * scale)


def _voigt_tensor(Cv):
    idx = {(0, 0): 0, (1, 1): 1, (2, 2): 2, (1, 2): 3, (2, 1): 3, (0, 2): 4, (2, 0): 4, (0, 1): 5, (1, 0): 5}
    C = np.zeros((3, 3, 3, 3))
    for i, j, k, l in np.ndindex(3, 3, 3, 3):
        C[i, j, k, l] = Cv[idx[(i, j)], idx[(k, l)]]
    return C


def _prim(a):
    return Atoms(numbers=[74], positions=[[0, 0, 0]], cell=0.5 * a * np.array([[-1, 1, 1], [1, -1, 1], [1, 1, -1]]), pbc=True)


def test_acoustic_slopes_match_christoffel_velocities(a0):
    calc = _calc(_unary_model())
    prim = _prim(a0)
    C = _voigt_tensor(_quiet_elastic(calc, prim)["C"])
    rho = W_MASS["W"] / abs(np.linalg.det(np.asarray(prim.get_cell())))      # amu / A^3
    kk = 2e-3                                                                  # 1 / A (without 2 pi)
    for n in (np.array([1.0, 0, 0]), np.array([1.0, 1.0, 0]) / np.sqrt(2)):
        gam = np.einsum("ijkl,j,l->ik", C, n, n)
        v_el = np.sqrt(np.linalg.eigvalsh(gam) * 1e9 / (rho * 1660.5390666))   # m / s
        q = np.asarray(prim.get_cell()) @ (kk * n)
        f = harmonic.phonon_frequencies(calc, prim, [q], n_super=6, masses=W_MASS)[0]
        v_ph = np.sort(f) * 1e12 / (kk * 1e10)
        assert np.allclose(v_ph, v_el, rtol=1e-3, atol=0), (n, v_ph, v_el)


def test_phonons_bcc_w(a0):
    calc = _calc(_unary_model())
    conv = _bcc(a0, (1, 1, 1))
    f0 = harmonic.phonon_frequencies(calc, conv, [[0, 0, 0]], n_super=5, masses=W_MASS)
    assert np.abs(f0[0, :3]).max() < 1e-5
    q = np.random.default_rng(2).uniform(-0.5, 0.5, (20, 3))
    f5 = harmonic.phonon_frequencies(calc, conv, q, n_super=5, masses=W_MASS)
    f6 = harmonic.phonon_frequencies(calc, conv, q, n_super=6, masses=W_MASS)
    assert np.abs(f5 - f6).max() <= 1e-8
    # the 1-atom primitive cell at the same Cartesian q: its 3 bands are among the conventional cell's 6
    prim = _prim(a0)
    kc = q @ np.linalg.inv(np.asarray(conv.get_cell())).T
    qp = kc @ np.asarray(prim.get_cell()).T
    fp = harmonic.phonon_frequencies(calc, prim, qp, n_super=6, masses=W_MASS)
    for k in range(len(q)):
        assert all(np.abs(f6[k] - x).min() <= 1e-8 for x in fp[k])
    fc, path_data, bands = calc.get_phonon_data(prim, n_super=6, resolution=10, masses=W_MASS)
    assert path_data["path"][0] == ("GAMMA", "H") and set(path_data["point_coords"]) == {"GAMMA", "H", "N", "P"}
    assert len(bands["frequencies"]) == 6 and bands["frequencies"][0].shape == (11, 3)
    assert bands["qpoints"][0].shape == (11, 3) and bands["distances"][0].shape == (11,)
    assert fc.shape == (1, 216, 3, 3)
    with pytest.raises(ValueError, match="harmonic: no masses"):
        calc.get_phonon_data(prim, n_super=2)


def test_abi_refusals():
    """The library's own checks, called directly (the Python layer refuses most of these before it)."""
    import ctypes as C
    from uf3_amd import _lib
    calc = _calc(_unary_model())
    ctx = _lib.get_context(calc.device)
    db = _lib.device_basis(calc.bspline_config, ctx)
    addr = _lib._addr
    atoms = _bcc(A0_W, (2, 2, 2))
    n = 16
    H = np.zeros(9 * n * n)
    Bo = np.zeros(36)

    def call(frames, lo, hi, born=False):
        batch = _lib.FrameBatch(frames)
        rc = ctx.lib.uf3_hessian(db.handle, C.byref(batch.struct), addr(batch.pos), addr(batch.z), calc._pc[0], calc._pc[1],
                                 calc._pc[2], lo, hi, addr(H), None, addr(Bo) if born else None)
        return rc, ctx.lib.uf3_last_error(ctx.handle).decode()

    assert call([atoms], 0, n, born=True)[0] == 0
    rc, msg = call([atoms, atoms], 0, n)
    assert rc == 1 and "exactly one frame" in msg
    for lo, hi in ((3, 3), (5, 2), (-1, 4), (0, n + 1)):
        rc, msg = call([atoms], lo, hi)
        assert rc == 1 and "row span" in msg, (lo, hi, msg)
    rc, msg = call([atoms], 0, 4, born=True)
    assert rc == 1 and "born" in msg
    far = np.asarray(atoms.get_positions()).copy()
    far[3] += 600 * np.asarray(atoms.get_cell())[0]
    rc, msg = call([Atoms(numbers=atoms.get_atomic_numbers(), positions=far, cell=atoms.get_cell(), pbc=True)], 0, n)
    assert rc == 1 and "500 cells" in msg
    bad = Atoms(numbers=[74, 42], positions=[[0, 0, 0], [1.6, 1.6, 1.6]], cell=np.eye(3) * 3.2, pbc=True)
    assert call([bad], 0, 2)[0] == 2
    with pytest.raises(_lib.SpeciesError):
        harmonic.hessian(calc, bad)
    with pytest.raises(ValueError, match="row span"):
        harmonic.hessian(calc, atoms, rows=(5, 5))
    with pytest.raises(ValueError, match="whole frame"):
        harmonic.hessian(calc, atoms, rows=(0, 4), strain=True)


def _abi(calc):
    from uf3_amd import _lib
    ctx = _lib.get_context(calc.device)
    return _lib, ctx, _lib.device_basis(calc.bspline_config, ctx)


def _w16():
    return synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=3)


def _w2():
    return synthetic.lattice_frame("bcc", (1, 1, 1), 3.165, [74], seed=4)


def _cluster13():
    pos = np.asarray(synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=7).get_positions(), dtype=float)
    keep = np.sort(np.argsort(np.linalg.norm(pos - pos.mean(axis=0), axis=1))[:13])
    return Atoms(numbers=np.full(13, 74), positions=pos[keep], cell=np.zeros((3, 3)), pbc=False)


def test_hessian_and_site_term_workspaces_stay_apart():
    """The Hessian's lists and the site terms' lists are two workspaces of one type: a site-term call on a batch of other sizes
    and another capacity between two Hessian calls changes no bit, on the host entries and with both device entries queued on
    one stream before anything waits (uf3_hessian_dev returns with k_hessian still to run on its lists)."""
    import ctypes as C
    import torch
    calc = _calc(_unary_model())
    _lib, ctx, db = _abi(calc)
    w16, others = _w16(), [_w2(), _cluster13()]
    H = harmonic.hessian(calc, w16)
    U, W = calc.site_terms(others)
    assert np.array_equal(harmonic.hessian(calc, w16), H)
    U2, W2 = calc.site_terms(others)
    assert all(np.array_equal(a, b) for a, b in zip(U + W, U2 + W2))
    # device entries, back to back on one stream
    dev = torch.device("cuda", calc.device if isinstance(calc.device, int) else 0)
    hb, sb = _lib.FrameBatch([w16]), _lib.FrameBatch(others)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    ptr = lambda t: C.c_void_p(t.data_ptr())                              # noqa: E731
    h_pos, h_z, s_pos, s_z = up(hb.pos), up(hb.z), up(sb.pos), up(sb.z)
    d_h = up(np.full(H.shape, -7.0))
    d_u, d_w = up(np.full(sb.n_atoms, -7.0)), up(np.full((sb.n_atoms, 9), -7.0))
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)
    prev = ctx.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            ctx.check(ctx.lib.uf3_hessian_dev(db.handle, C.byref(hb.struct), ptr(h_pos), ptr(h_z), calc._pc[0], calc._pc[1],
                                              calc._pc[2], 0, 16, ptr(d_h), None, None))
            ctx.check(ctx.lib.uf3_site_terms_dev(db.handle, C.byref(sb.struct), ptr(s_pos), ptr(s_z), calc._pc[0], calc._pc[1],
                                                 calc._pc[2], ptr(d_u), ptr(d_w)))
            stream.synchronize()
    finally:
        ctx.restore_stream(prev)
    assert np.array_equal(d_h.cpu().numpy(), H)
    assert np.array_equal(d_u.cpu().numpy(), np.concatenate(U))
    assert np.array_equal(d_w.cpu().numpy().reshape(-1, 3, 3), np.concatenate(W))


@pytest.mark.parametrize("label", ["w2", "nexe4"])
def test_optional_outputs_do_not_move_the_hessian(label):
    """uf3_hessian's staging block holds mixed and born only when they are asked for: hess has the same bits with and without
    either, and each optional output the same bits whatever else is asked for."""
    import ctypes as C
    if label == "w2":
        calc, atoms = _calc(_unary_model()), _w2()
    else:
        calc = _calc(ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_binary.json")))
        atoms = synthetic.lattice_frame("fcc", (1, 1, 1), 4.6, [10, 54], seed=5)
    _lib, ctx, db = _abi(calc)
    batch = _lib.FrameBatch([atoms])
    n = batch.n_atoms
    assert n == (2 if label == "w2" else 4)
    addr = _lib._addr
    got = {}
    for want_m in (False, True):
        for want_b in (False, True):
            H, M, B = np.full((3 * n, 3 * n), -7.0), np.full((3 * n, 6), -7.0), np.full((6, 6), -7.0)
            ctx.check(ctx.lib.uf3_hessian(db.handle, C.byref(batch.struct), addr(batch.pos), addr(batch.z), calc._pc[0], calc._pc[1],
                                          calc._pc[2], 0, n, addr(H), addr(M) if want_m else None, addr(B) if want_b else None))
            assert want_m or np.all(M == -7.0)
            assert want_b or np.all(B == -7.0)
            got[want_m, want_b] = (H, M, B)
    H0 = got[False, False][0]
    assert np.abs(H0).max() > 0 and np.all(H0 != -7.0)
    assert all(np.array_equal(g[0], H0) for g in got.values())
    assert np.array_equal(got[True, False][1], got[True, True][1]) and np.all(got[True, True][1] != -7.0)
    assert np.array_equal(got[False, True][2], got[True, True][2]) and np.all(got[True, True][2] != -7.0)


def test_the_site_term_kernel_s_neighbour_limit_is_not_the_hessian_s():
    """12 288 neighbours of one atom is the size of k_flux_site_terms' LDS index array, not a property of the lists both entries
    build: one Xe atom in a 0.5 A cell has some 16 000 images inside the pair range (3 A < r < 8 A, 16 images tried per side),
    uf3_site_terms refuses it by that name, and uf3_hessian, whose kernel walks the list from global memory, takes it."""
    from uf3_amd import _lib
    calc = _calc(ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_binary.json")))
    atoms = Atoms(numbers=[54], positions=[[0.1, 0.2, 0.3]], cell=np.eye(3) * 0.5, pbc=True)
    with pytest.raises(_lib.UF3Error, match="more than 12288 neighbours"):
        calc.site_terms([atoms])
    H = harmonic.hessian(calc, atoms)
    assert H.shape == (3, 3) and np.all(np.isfinite(H))
