"""
Leverage on the device (``uf3_leverage[_dev]``, ``WeightedLinearModel.leverage``, ``pipeline.DeviceLeverage``,
``UFCalculator.get_leverages``): q = |W x|^2 per row or per atom, W the inverse Cholesky factor of the system the fit solved.

Every numerical comparison is ``|q - leverage_reference| <= leverage_bound`` row by row: the bound is the first-order rounding
bound of any summation order of the same products (least_squares.leverage_bound), about 1e-12 of q on the fixture -- nothing
here is a measured tolerance.  The host side (whitening, posterior file, errors) is tests/test_leverage_host.py.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from uf3_amd import _lib, pipeline, synthetic
from uf3_amd.forcefield import calculator
from uf3_amd.regression import least_squares as ls
from uf3_amd.representation import process
from _util import GOLDEN
from test_leverage_host import fixture_model

pytestmark = pytest.mark.gpu
UF3_EINVAL = 1


def _within(q, x, w, group, label):
    ref, bound = ls.leverage_reference(x, w, group), ls.leverage_bound(x, w, group)
    worst = float((np.abs(q - ref) / np.where(bound > 0, bound, 1.0)).max()) if len(ref) else 0.0
    print(f"\n{label}: {len(ref)} outputs, worst |q - ref| / bound = {worst:.3e}, bound / q ~ {float(np.median(bound / np.where(ref > 0, ref, 1.0))):.1e}")
    assert q.shape == ref.shape
    assert np.all(np.abs(q - ref) <= bound), label


def _host_entry(x, n_rows, n_feat, ld, w, group, q=None):
    """``uf3_leverage`` on a [n_rows, ld] host array -> (return code, q)"""
    ctx = _lib.get_context()
    q = np.full(n_rows // group if group in (1, 3) and n_rows % group == 0 else n_rows, -7.0) if q is None else q
    rc = ctx.lib.uf3_leverage(ctx.handle, _lib._p(x), n_rows, n_feat, ld, _lib._p(w), group, _lib._p(q))
    return rc, q


# ---------------------------------------------------------------------------------------------- 1, 2: the fixture
def test_fixture_rows_through_the_model():
    d, model, *_ = fixture_model()
    w = model.whitening()
    _within(model.leverage(d["x_e"]), d["x_e"], w, 1, "x_e 40 x 73, group 1")
    _within(model.leverage(d["x_f"]), d["x_f"], w, 1, "x_f 900 x 73, group 1")
    _within(model.leverage(d["x_f"], group=3), d["x_f"], w, 3, "x_f 900 x 73, group 3")
    _within(model.leverage(d["x_f"].reshape(300, 3, 73), group=3), d["x_f"], w, 3, "x_f 300 x 3 x 73, group 3")


def test_trace_identity_without_the_whitening_matrix():
    """Weighted training leverages sum to the effective number of parameters: with A = G + R^T R and G the weighted Gram,
    kappa w_e^2 sum q_e + (1 - kappa) w_f^2 sum q_f = tr(A^-1 G) = K - tr(A^-1 R^T R).  The right side never sees W."""
    d, model, kappa, w_e, w_f = fixture_model()
    a, mask = model.system_matrix, np.asarray(model.mask)
    reg = d["regularizer"][:, mask]
    want = len(mask) - np.trace(np.linalg.solve(a, reg.T @ reg))
    got = kappa * w_e ** 2 * model.leverage(d["x_e"]).sum() + (1 - kappa) * w_f ** 2 * model.leverage(d["x_f"], group=3).sum()
    print(f"\ntrace identity: device {got!r}, NumPy {want!r}, relative difference {abs(got - want) / want:.2e}")
    assert abs(got - want) <= 1e-9 * abs(want)


# ---------------------------------------------------------------------------------------------- 3, 4: shapes
N_FEATS = [1, 3, 15, 16, 17, 33, 70, 434, 1798]
N_ROWS = [1, 3, 47, 48, 49, 144, 333]


@functools.lru_cache(maxsize=None)
def _synthetic(n_feat):
    """(X [333, n_feat] with half the entries zero and two all-zero rows, W [n_feat, n_feat], frozen indices): W from a seeded SPD
    matrix with condition number 1e3 on the unfrozen columns, embedded with zero rows and columns at the frozen ones; X holds
    finite non-zero values in the frozen columns.  Frozen: none at n_feat = 1, two up to 16 columns, three beyond."""
    rng = np.random.default_rng(1000 + n_feat)
    n_frozen = 0 if n_feat < 3 else (2 if n_feat <= 16 else 3)
    frozen = np.sort(rng.choice(n_feat, n_frozen, replace=False)) if n_frozen else np.zeros(0, dtype=int)
    mask = np.setdiff1d(np.arange(n_feat), frozen)
    k = len(mask)
    qm, _ = np.linalg.qr(rng.normal(size=(k, k)))
    a = (qm * np.logspace(0, 3, k)) @ qm.T if k > 1 else np.array([[2.5]])
    a = 0.5 * (a + a.T)
    w = np.zeros((n_feat, n_feat))
    w[np.ix_(mask, mask)] = np.tril(np.linalg.solve(np.linalg.cholesky(a), np.eye(k)))
    x = rng.normal(size=(333, n_feat)) * (rng.random((333, n_feat)) < 0.5)
    x[:, frozen] = rng.uniform(1.0, 9.0, (333, len(frozen)))
    for r in (1, 331):
        x[r] = 0.0
    return x, w, frozen


@pytest.mark.parametrize("n_feat", N_FEATS)
def test_shapes_where_the_tiling_can_go_wrong(n_feat):
    x_all, w, frozen = _synthetic(n_feat)
    rows = [48, 333] if n_feat == 1798 else N_ROWS
    for n_rows in rows:
        x = np.ascontiguousarray(x_all[:n_rows])
        for pad in (0, 5):
            ld = n_feat + pad
            xp = np.full((n_rows, ld), np.nan)
            xp[:, :n_feat] = x
            for group in (1, 3):
                if n_rows % group:
                    continue
                label = f"n_feat {n_feat}, n_rows {n_rows}, ld {ld}, group {group}"
                rc, q = _host_entry(xp, n_rows, n_feat, ld, w, group)
                assert rc == 0, label
                assert np.all(np.isfinite(q)) and np.all(q >= 0), label
                zero = ~x.reshape(-1, group * n_feat).any(axis=1)
                assert np.all(q[zero] == 0.0), label
                if n_rows > 1 and group == 1:
                    assert zero[1]
                _within(q, x, w, group, label)
                rc, again = _host_entry(xp, n_rows, n_feat, ld, w, group)
                assert rc == 0 and np.array_equal(q, again), label + ": a second call differs"


def test_rows_do_not_depend_on_their_neighbours():
    for n_feat in (70, 434):
        x, w, _ = _synthetic(n_feat)
        bound1 = ls.leverage_bound(x, w, 1)
        q_all = _host_entry(x, 333, n_feat, n_feat, w, 1)[1]
        q_48 = _host_entry(np.ascontiguousarray(x[:48]), 48, n_feat, n_feat, w, 1)[1]
        assert np.all(np.abs(q_48 - q_all[:48]) <= bound1[:48])
        q_3 = _host_entry(x, 333, n_feat, n_feat, w, 3)[1]
        assert np.all(np.abs(q_3 - q_all.reshape(-1, 3).sum(1)) <= ls.leverage_bound(x, w, 3))


# ---------------------------------------------------------------------------------------------- 5: the device entry
def test_device_entry_on_a_torch_stream():
    import torch
    n_feat = 434
    x, w, _ = _synthetic(n_feat)
    ctx = _lib.get_context()
    dev = torch.device("cuda", ctx.device)
    host = {g: _host_entry(x, 333, n_feat, n_feat, w, g)[1] for g in (1, 3)}
    d_x, d_w = torch.from_numpy(x).to(dev), torch.from_numpy(w).to(dev)
    d_q = torch.from_numpy(np.full(333, -7.0)).to(dev)            # (copies only: no torch kernel takes part)
    torch.cuda.synchronize(dev)
    stream = torch.cuda.Stream(dev)

    def call(n_rows, group, feat=n_feat):
        return ctx.lib.uf3_leverage_dev(ctx.handle, C.c_void_p(d_x.data_ptr()), n_rows, feat, n_feat, C.c_void_p(d_w.data_ptr()), group,
                                        C.c_void_p(d_q.data_ptr()))

    prev = ctx.set_stream(stream.cuda_stream)
    try:
        with torch.cuda.stream(stream):
            assert call(0, 1) == 0 and call(0, 3) == 0
            stream.synchronize()
            assert np.all(d_q.cpu().numpy() == -7.0)                 # n_rows = 0 launches nothing
            assert call(333, 2) == UF3_EINVAL
            assert call(332, 3) == UF3_EINVAL
            assert call(333, 1, feat=0) == UF3_EINVAL
            stream.synchronize()
            assert np.all(d_q.cpu().numpy() == -7.0)
            for group in (1, 3):
                assert call(333, group) == 0
                stream.synchronize()
                got = d_q.cpu().numpy()[:333 // group]
                assert np.array_equal(got, host[group]), f"group {group}: the device entry differs from the host entry"
    finally:
        ctx.restore_stream(prev)
    assert _host_entry(x, 333, n_feat, n_feat, w, 2)[0] == UF3_EINVAL
    assert _host_entry(x, 332, n_feat, n_feat, w, 3)[0] == UF3_EINVAL


def test_launch_report(monkeypatch, capfd):
    monkeypatch.setenv("UF3_DEBUG_LDS", "1")
    monkeypatch.setattr(_lib, "_contexts", {})
    x, w, _ = _synthetic(70)
    assert _host_entry(x, 333, 70, 70, w, 3)[0] == 0
    err = capfd.readouterr().err
    assert "uf3: leverage kernel=k_leverage rows=333 feat=70 ld=70 group=3 blocks=7 rows_per_block=48" in err, err


# ---------------------------------------------------------------------------------------------- 6 - 8: frames
def _seeded_fit(basis, frames, seed, **reg):
    fz = process.BasisFeaturizer(basis)
    x_e, x_f, _ = fz.featurize_frames(frames)
    rng = np.random.default_rng(seed)
    y_e = rng.normal(-8.9, 0.05, len(frames))
    y_f = rng.normal(0.0, 0.5, x_f.shape[0] * 3)
    model = ls.WeightedLinearModel(basis, **reg)
    model.fit(x_e / np.array([len(a) for a in frames])[:, None], y_e, x_f.reshape(-1, x_f.shape[-1]), y_f, weight=0.5)
    return model, fz


@functools.lru_cache(maxsize=None)
def _ragged_case():
    frames = [synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=1),
              synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [42, 74], seed=2),
              synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [42, 74], seed=3),
              synthetic.lattice_frame("bcc", (4, 4, 4), 3.165, [42, 74], seed=4),
              synthetic.lattice_frame("bcc", (3, 3, 3), 3.165, [74], seed=5),
              synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [42, 74], seed=6)]
    basis = synthetic.notebook_basis(['Mo', 'W'])
    model, fz = _seeded_fit(basis, frames, 11)
    return frames, basis, model, fz


def _host_route(model, fz, frames):
    x_e, x_f, offsets = fz.featurize_frames(frames)
    x_e = x_e / np.array([len(a) for a in frames])[:, None]
    return x_e, x_f.reshape(-1, x_f.shape[-1]), offsets


def test_device_leverage_against_the_host_route():
    frames, basis, model, fz = _ragged_case()
    assert [len(a) for a in frames] == [16, 54, 16, 128, 54, 16]
    x_e, x_f, offsets = _host_route(model, fz, frames)
    w = model.whitening()
    lev = pipeline.DeviceLeverage(model, fz, max_atoms_per_chunk=100)     # chunks 16 + 54 + 16 | 128 (over the limit) | 54 + 16
    out = lev.frames(frames)
    assert sorted(out) == ["energy", "force", "offsets"]
    assert np.array_equal(out["offsets"], offsets) and out["offsets"].dtype == np.int64
    assert out["energy"].shape == (6,) and out["force"].shape == (284,)
    _within(out["energy"], x_e, w, 1, "DeviceLeverage energy rows")
    _within(out["force"], x_f, w, 3, "DeviceLeverage force rows")
    # ... and the host route through the model agrees with the same reference
    _within(model.leverage(x_e), x_e, w, 1, "model.leverage energy rows")
    _within(model.leverage(x_f, group=3), x_f, w, 3, "model.leverage force rows")
    only_e = lev.frames(frames, forces=False)
    assert sorted(only_e) == ["energy", "offsets"]
    # (another featurizer call: its energy rows are sums of atomic adds, equal up to their order -- the bound, not bit for bit)
    _within(only_e["energy"], x_e, w, 1, "DeviceLeverage energy rows, forces=False")
    one = pipeline.DeviceLeverage(model, fz).frames(frames)             # one chunk
    _within(one["force"], x_f, w, 3, "DeviceLeverage force rows, one chunk")
    _within(one["energy"], x_e, w, 1, "DeviceLeverage energy rows, one chunk")


@functools.lru_cache(maxsize=None)
def _w_case():
    basis = synthetic.notebook_basis(['W'])
    train = [synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=s, rattle=0.08) for s in range(12)]
    model, fz = _seeded_fit(basis, train, 7, ridge_1b=1e-8, ridge_2b=1e-8, ridge_3b=1e-8, curvature_2b=1e-8)
    return basis, train, model, fz


def test_it_tells_seen_from_unseen():
    """A held-out frame drawn like the training frames lies inside the training leverages; the same frame compressed to
    a = 2.85 A lies far outside (on the CPU, from the oracle's rows: 0.63 x, 0.22 x and 374 x the training maxima)."""
    basis, train, model, fz = _w_case()
    lev = pipeline.DeviceLeverage(model, fz)
    tr = lev.frames(train)
    held = lev.frames([synthetic.lattice_frame("bcc", (2, 2, 2), 3.165, [74], seed=99, rattle=0.08)])
    squeezed = lev.frames([synthetic.lattice_frame("bcc", (2, 2, 2), 2.85, [74], seed=99, rattle=0.08)])
    e_max, f_max = tr["energy"].max(), tr["force"].max()
    print(f"\nheld-out: energy {held['energy'][0] / e_max:.3f} x, largest force {held['force'].max() / f_max:.3f} x the training maximum; "
          f"compressed: smallest force {squeezed['force'].min() / f_max:.1f} x")
    assert held["energy"][0] < e_max
    assert np.all(held["force"] < f_max)
    assert np.all(squeezed["force"] > 10 * f_max)


def test_calculator_get_leverages():
    basis, train, model, fz = _w_case()
    calc = calculator.UFCalculator(model)
    want = pipeline.DeviceLeverage(model, fz).frames(train[:3])
    got = calc.get_leverages(train[:3])
    # (two featurizer calls: rows equal up to the order of their atomic adds, so "equal" is the bound of every comparison here)
    x_e, x_f, offsets = _host_route(model, fz, train[:3])
    w = model.whitening()
    b_e, b_f = ls.leverage_bound(x_e, w, 1), ls.leverage_bound(x_f, w, 3)
    assert sorted(got) == ["energy", "force", "offsets"] and np.array_equal(got["offsets"], want["offsets"])
    assert got["energy"].shape == (3,) and got["force"].shape == (48,)
    assert np.all(np.abs(got["energy"] - want["energy"]) <= b_e) and np.all(np.abs(got["force"] - want["force"]) <= b_f)
    one = calc.get_leverages(train[1])
    assert isinstance(one["energy"], float) and abs(one["energy"] - want["energy"][1]) <= b_e[1]
    assert one["force"].shape == (16,) and np.all(np.abs(one["force"] - want["force"][16:32]) <= b_f[16:32])
    assert np.array_equal(one["offsets"], [0, 16])
    bare = calculator.UFCalculator(ls.WeightedLinearModel.from_json(os.path.join(GOLDEN, "model_unary.json")))
    with pytest.raises(ValueError, match="load_posterior"):
        bare.get_leverages(train[0])
