"""The bases and frames of tests/_uneven.py do what tests/test_gpu_uneven_legs.py needs of them, and the references that test
holds the kernels to agree with each other there.  No GPU.

Bounds between the references (fp64 sums of 1e3 to 1e4 terms taken in different orders, two independent B-spline codes):
1e-11 of the quantity's largest magnitude.  Central differences with step h carry h^2 f''' / 6 and eps |f| / h: 1e-6 of the
largest entry at h = 1e-4 (energies) and h = 1e-5 (forces), the bound tests/test_gpu_harmonic.py gives differences of forces."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
import _flux_ref as FR
import _harmonic_ref as HR
import _uneven as U
from _util import tensor_to_voigt

RTOL = 1e-11
FD_TOL = 1e-6


@functools.lru_cache(maxsize=None)
def _ob(name):
    return O.OracleBasis(U.basis(name))


def _coeff(name):
    return U.coefficients(U.basis(name))


def test_the_bases_are_what_they_claim():
    for name in ("uneven_lead0", "uneven_lead3"):
        b = U.basis(name)
        trios = b.interactions_map[3]
        assert len(trios) == 18 and int(b.leading_trim[3]) == int(name[-1]) and int(b.trailing_trim[3]) == 3
        assert len({(tuple(b.r_min_map[t]), tuple(b.r_max_map[t]), tuple(b.resolution_map[t])) for t in trios}) == 18
        assert len({(b.r_min_map[p], b.r_max_map[p], b.resolution_map[p]) for p in b.interactions_map[2]}) == 6
        for t in trios:
            lo, hi, res = b.r_min_map[t], b.r_max_map[t], b.resolution_map[t]
            same = lo[0] == lo[1] and hi[0] == hi[1] and res[0] == res[1]
            assert same == (t[1] == t[2]) and b.symmetry[t] == (2 if t[1] == t[2] else 1), t
            assert 0.7 * (hi[0] + hi[1]) <= hi[2] <= 0.9 * (hi[0] + hi[1]) and 1.6 <= lo[2] <= 2.6
    for name in ("sym1_unary", "sym1_binary"):
        b = U.basis(name)
        for t in b.interactions_map[3]:
            assert b.symmetry[t] == 1 and list(b.r_max_map[t]) == [3.2, 3.8, 6.4] and list(b.resolution_map[t]) == [4, 5, 8]
    for name in U.BASES:
        for a in U.all_frames(name):
            assert 16 <= len(a) <= 54 and U.inside_cell(a)
        assert len({len(a) for a in U.frames(name)}) == len(U.frames(name))                  # a ragged batch


@pytest.mark.parametrize("name", U.BASES)
def test_liveness(name):
    """uneven: each of the six masks rejects, and enough triplets pass; sym-1: triplets whose two assignments differ"""
    for a in U.all_frames(name):
        c = U.leg_census(_ob(name), a)
        print(name, len(a), c)
        if name.startswith("uneven"):
            assert set(np.asarray(a.get_atomic_numbers()).tolist()) == set(U.UNEVEN_NUMBERS)
            assert all(c[k] >= 5 for k in ("l_lower", "l_upper", "m_lower", "m_upper", "n_lower", "n_upper")), c
            assert c["accepted"] >= 500, c
        else:
            assert c["ambiguous"] >= 50, c


@pytest.mark.parametrize("name", U.BASES)
def test_sensitivity(name):
    """the error the GPU tests look for is visible: legs exchanged (uneven) or the equal-species order reversed (sym-1)"""
    ob, coeff = _ob(name), _coeff(name)
    for a in U.all_frames(name):
        e, f = U.restated(ob, a, coeff)
        e_o = O.evaluate(ob, a, coeff)[0]
        assert abs(e - e_o) <= RTOL * max(1.0, abs(e_o))                                     # the restatement itself is right
        e_x, f_x = U.restated(ob, a, coeff, "exchange_lm" if name.startswith("uneven") else "reverse_equal")
        de, df = abs(e_x - e) / abs(e), np.abs(f_x - f).max() / np.abs(f).max()
        print(f"{name} {len(a)} atoms: wrong assignment moves E by {de:.2e} relative, F by {df:.2e} of max|F|")
        assert de > 1e-3 and df > 1e-3


@pytest.mark.parametrize("name", U.BASES)
def test_references_agree_on_energy_forces_and_virial(name):
    ob, coeff = _ob(name), _coeff(name)
    a = U.small_frame(name)
    n = len(a)
    e_o, f_o, v_o = O.evaluate(ob, a, coeff, virial=True)
    Us, W = FR.site_terms(ob, a, coeff)
    assert abs(Us.sum() - e_o) <= RTOL * max(1.0, np.abs(Us).sum())
    Ws = W.sum(axis=0)
    assert np.abs(tensor_to_voigt(0.5 * (Ws + Ws.T)) - v_o).max() <= RTOL * np.abs(v_o).max()
    f_t = FR.term_forces(ob, a, coeff)
    e_r, f_r = U.restated(ob, a, coeff)
    assert np.abs(f_r - f_t).max() <= RTOL * np.abs(f_t).max()
    # minus the gradient of the oracle's energy, by central differences
    h = 1e-4
    pos = np.asarray(a.get_positions(), dtype=float)
    fd = np.zeros((n, 3))
    for k in range(3 * n):
        e_pm = []
        for sgn in (1, -1):
            p = pos.copy()
            p[k // 3, k % 3] += sgn * h
            e_pm.append(O.evaluate(ob, U.displaced(a, p), coeff, forces=False)[0])
        fd[k // 3, k % 3] = -(e_pm[0] - e_pm[1]) / (2 * h)
    err = np.abs(f_t - fd).max() / np.abs(fd).max()
    dev = np.abs(f_o - f_t).max() / np.abs(f_t).max()
    print(f"{name}: term_forces against differences of the oracle energy {err:.2e}; oracle forces against term_forces {dev:.2e}")
    assert err <= FD_TOL
    if name.startswith("uneven"):
        assert dev <= RTOL                      # neighbour species differ wherever the legs do: nothing to choose
    else:
        assert dev > 1e-3                       # the reference's forces on a symmetry-1 trio are not its energy's gradient


@pytest.mark.parametrize("name", U.BASES)
def test_oracle_forces_are_the_term_forces_on_every_uneven_frame(name):
    """what tests/test_gpu_uneven_legs.py holds the forces to is one thing on the uneven bases (no ghost-centred term lost to
    the oracle's image range on these cells) and the energy's gradient, not the oracle's forces, on the sym-1 bases"""
    ob, coeff = _ob(name), _coeff(name)
    for a in U.frames(name):
        f_o = O.evaluate(ob, a, coeff)[1]
        f_t = FR.term_forces(ob, a, coeff)
        dev = np.abs(f_o - f_t).max() / np.abs(f_t).max()
        print(f"{name} {len(a)} atoms: oracle forces against term_forces {dev:.2e}")
        assert (dev <= RTOL) if name.startswith("uneven") else (dev > 1e-3)


def _fd_frame(name):
    """four atoms, 1 x 1 x 2 cells: every atom neighbours its own images"""
    if name.startswith("uneven"):
        return U._bcc(U.UNEVEN_NUMBERS, (1, 1, 2), 2.65, 41, 0.12)
    return U._bcc([74] if name == "sym1_unary" else [42, 74], (1, 1, 2), 3.165, 42, 0.08)


@pytest.mark.parametrize("name", U.BASES)
def test_restated_hessian_is_the_derivative_of_the_term_forces(name):
    ob, coeff = _ob(name), _coeff(name)
    a = _fd_frame(name)
    n = len(a)
    H = HR.hessian(ob, a, coeff)[0]
    h = 1e-5
    pos = np.asarray(a.get_positions(), dtype=float)
    Hfd = np.zeros((3 * n, 3 * n))
    for k in range(3 * n):
        f_pm = []
        for sgn in (1, -1):
            p = pos.copy()
            p[k // 3, k % 3] += sgn * h
            f_pm.append(FR.term_forces(ob, U.displaced(a, p), coeff).ravel())
        Hfd[:, k] = -(f_pm[0] - f_pm[1]) / (2 * h)
    err = np.abs(H - Hfd).max() / np.abs(H).max()
    print(f"{name}: restated Hessian against differences of term_forces {err:.2e}")
    assert err <= FD_TOL
