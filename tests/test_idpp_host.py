"""What the NumPy restatement of the image dependent pair potential (tests/_idpp_ref.py) proves without a device: its force is
the gradient of its S, S vanishes exactly at both end points, the parity inputs of tests/test_gpu_idpp.py are conditioned as
that file needs them, and ``IDPP`` / ``idpp_interpolate`` refuse bad arguments before any device call."""
import numpy as np
import pytest

from uf3_amd import _lib
from uf3_amd.data.atoms import Atoms
from uf3_amd.forcefield import neb
import _idpp_ref as I

MARGIN = 1e-6


def _cluster(seed, cell, pbc):
    """Three images' worth of positions (image, first, last) of 9 atoms spread over about a cell."""
    rng = np.random.default_rng(seed)
    frac = rng.random((9, 3))
    box = np.asarray(cell, float) if np.any(pbc) else 5.0 * np.eye(3)
    x0 = frac @ box
    x1 = x0 + rng.normal(0, 0.4, x0.shape)
    x = 0.6 * x0 + 0.4 * x1 + rng.normal(0, 0.2, x0.shape)
    return x, x0, x1


CUBE = 5.0 * np.eye(3)
CELLS = {"cubic": (CUBE, [True, True, True]), "skewed": (I.SKEW @ CUBE, [True, True, True]),
         "slab": (np.array([[5.0, 0.0, 0.0], [5.0, 5.0, 0.0], [0.0, 0.0, 5.0]]), [True, True, False]),    # (skewed in its plane)
         "cluster": (np.zeros((3, 3)), [False, False, False])}


@pytest.mark.parametrize("name", list(CELLS))
def test_force_is_the_gradient_of_S(name):
    cell, pbc = CELLS[name]
    x, x0, x1 = _cluster(7, cell, pbc)
    lam, h = 0.4, 1e-5
    S, F = I.image_terms(x, x0, x1, lam, cell, pbc)
    num = np.zeros_like(F)
    for i in range(len(x)):
        for k in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, k] += h
            xm[i, k] -= h
            num[i, k] = -(I.image_terms(xp, x0, x1, lam, cell, pbc)[0] - I.image_terms(xm, x0, x1, lam, cell, pbc)[0]) / (2 * h)
    err = np.abs(F - num).max() / np.abs(F).max()
    print(f"idpp force against central differences, {name}: {err:.3g} (S {S:.4g}, largest |F| {np.abs(F).max():.4g})")
    assert S > 0 and err <= 1e-6
    # the longdouble variant is the same function
    SL, FL = I.image_terms(x, x0, x1, lam, cell, pbc, dtype=np.longdouble)
    assert abs(float(SL) - S) <= 1e-13 * S and np.abs(np.asarray(FL, float) - F).max() <= 1e-13 * np.abs(F).max()


def test_nearest_images_are_nearest():
    rng = np.random.default_rng(3)
    for name, (cell, pbc) in CELLS.items():
        D = rng.uniform(-5.0, 5.0, (200, 3))                             # (fractions within -3 .. 3 of every cell here)
        v = I.nearest(D, cell, pbc)
        per = np.flatnonzero(pbc)
        best = np.full(len(D), np.inf)
        for s in np.ndindex(*([7] * len(per))):                        # brute force over -3 .. 3 cells
            shift = sum(((s[q] - 3) * np.asarray(cell, float)[per[q]] for q in range(len(per))), np.zeros(3))
            best = np.minimum(best, np.linalg.norm(D + shift, axis=1))
        assert np.abs(np.linalg.norm(v, axis=1) - best).max() <= 1e-12, name
    assert I.orthogonal(CUBE, [True] * 3) and not I.orthogonal(I.SKEW @ CUBE, [True] * 3)


def test_S_vanishes_exactly_at_both_end_points():
    bands = I.batch()
    S, F = I.evaluate_bands(bands)
    _, off, first, _, _ = I.layout(bands)
    for k in range(len(bands)):
        for f in (first[k], first[k + 1] - 1):
            assert S[f] == 0.0 and np.all(F[off[f]:off[f + 1]] == 0.0), (k, f)
    assert [(len(b), len(b[0])) for b in bands] == [(3, 2), (3, 1), (4, 257), (5, 53), (4, 54), (6, 16)]


@pytest.mark.parametrize("name", list(I.PARITY))
def test_the_parity_inputs_are_well_conditioned(name):
    r = I.parity_run(name)
    print(f"idpp restatement {name}: smallest margin {r['margins'].min():.3g} 1/A^2, steps {r['steps'].tolist()}, "
          f"criterion {r['crit'].tolist()}")
    assert r["margins"].min() >= MARGIN                                  # every ordering of S a band branched on is clear
    assert r["status"].tolist() == [1] and r["steps"][0] <= 400          # converged at fmax 1e-2 (30 + 400 evaluations)


def test_the_straight_exchange_is_what_the_device_test_needs():
    ini, fin = I.straight_exchange_ends()
    d = I.min_distances(neb.interpolate(ini, fin, 7))
    assert len(ini) == 54 and d[3] < 0.05 and min(d[0], d[-1]) > 2.5, d


def test_arguments_are_refused_before_the_device_is_touched(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "get_context", no_device)
    band = I.exchange16(4)
    ok = lambda **kw: neb.IDPP(band, **kw)
    with pytest.raises(ValueError, match="IDPP: band 0 has 2 images"):
        neb.IDPP(band[:2])
    with pytest.raises(ValueError, match="IDPP: bands must be"):
        neb.IDPP(band[0])
    other = Atoms(numbers=band[1].get_atomic_numbers()[::-1], positions=band[1].get_positions(), cell=band[1].get_cell(), pbc=True)
    with pytest.raises(ValueError, match="IDPP: band 0, image 1: species"):
        neb.IDPP([band[0], other, band[2]])
    with pytest.raises(ValueError, match="IDPP: band 0, image 2: positions identical"):
        neb.IDPP([band[0], band[1], band[1], band[3]])
    for bad in (0.0, -1.0, np.inf, [0.1, 0.2]):
        with pytest.raises(ValueError, match="IDPP: spring"):
            ok(spring=bad)
    with pytest.raises(ValueError, match="IDPP: fixed"):
        ok(fixed=np.zeros(5, bool))
    mask = np.zeros(64, bool)
    mask[3] = True
    with pytest.raises(ValueError, match="IDPP: band 0, image 1: fixed mask differs"):
        ok(fixed=mask)
    with pytest.raises(ValueError, match="IDPP: device"):
        ok(device=-1)
    with pytest.raises(AssertionError, match="the device was touched"):
        ok()                                                             # good arguments: the first touch of the device
    a, b = band[0], band[-1]
    for kw, what in ((dict(n_images=2), "n_images"), (dict(n_images=5, fmax=0.0), "fmax"), (dict(n_images=5, max_steps=-1), "max_steps"),
                     (dict(n_images=5, climb=True), "unknown arguments"), (dict(n_images=5, spring=-1.0), "spring")):
        with pytest.raises(ValueError, match=what):
            neb.idpp_interpolate(a, b, **kw)
    with pytest.raises(ValueError, match="idpp_interpolate: initial and final"):
        neb.idpp_interpolate([a, a], [b], 5)
    with pytest.raises(ValueError, match="idpp_interpolate: initial and final"):
        neb.idpp_interpolate([a], b, 5)
    with pytest.raises(AssertionError, match="the device was touched"):
        neb.idpp_interpolate([a, a], [b, b], 5)
