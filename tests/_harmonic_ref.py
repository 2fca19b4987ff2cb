"""NumPy restatement of the analytic Hessian (uf3_amd/csrc/uf3_hessian.h) over the oracle's explicit supercell, for frames of
<= 64 atoms: H [3N, 3N], mixed [3N, 6] = d2E / dx dt_v and born [6, 6] = d2E / dt_u dt_v, from the B-spline basis functions
with nu = 0, 1, 2 and the chain rule term by term (every term whole, not row by row), for tests/test_harmonic_host.py and
tests/test_gpu_harmonic.py."""
import numpy as np
from scipy.interpolate import BSpline

from oracle import oracle as O

_VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def _basis(knots, x, nu):
    knots = np.asarray(knots, dtype=float)
    nb = len(knots) - 4
    return BSpline(knots, np.eye(nb), 3, extrapolate=False)(np.atleast_1d(x), nu=nu)


def _strain_dir(v, d):
    o = np.zeros(3)
    a, b = _VOIGT[v]
    if a == b:
        o[a] = d[a]
    else:
        o[a], o[b] = 0.5 * d[b], 0.5 * d[a]
    return o


def _add(H, L, B, par, legs, d, g, K):
    """One term: slots' parents par, legs (from, to), vectors d [nl, 3], leg gradient g [nl], leg Hessian K [nl, nl]."""
    nl, ns = len(legs), len(par)
    r = np.linalg.norm(d, axis=1)
    u = d / r[:, None]
    sg = np.zeros((nl, ns))
    for q, (f, t) in enumerate(legs):
        sg[q, t] += 1.0
        sg[q, f] -= 1.0
    P = [np.eye(3) - np.outer(u[q], u[q]) for q in range(nl)]
    for s in range(ns):
        for t in range(ns):
            blk = np.zeros((3, 3))
            for q in range(nl):
                for q2 in range(nl):
                    blk += K[q, q2] * sg[q, s] * sg[q2, t] * np.outer(u[q], u[q2])
                blk += g[q] * sg[q, s] * sg[q, t] * P[q] / r[q]
            H[3 * par[s]:3 * par[s] + 3, 3 * par[t]:3 * par[t] + 3] += blk
    w = np.array([[d[q, a] * d[q, b] / r[q] for (a, b) in _VOIGT] for q in range(nl)])      # [nl, 6]
    kw = K @ w
    for s in range(ns):
        for v in range(6):
            acc = np.zeros(3)
            for q in range(nl):
                ed = _strain_dir(v, d[q])
                acc += sg[q, s] * (u[q] * kw[q, v] + g[q] * (P[q] @ ed) / r[q])
            L[3 * par[s]:3 * par[s] + 3, v] += acc
    # d2 r / dt_u dt_v = (E_u d) . (E_v d) / r - w_u w_v / r  (d = (I + eps) d0: the vector is linear in t)
    for v1 in range(6):
        for v2 in range(6):
            acc = 0.0
            for q in range(nl):
                dw = (_strain_dir(v1, d[q]) @ _strain_dir(v2, d[q]) - w[q, v1] * w[q, v2]) / r[q]
                acc += w[q, v1] * kw[q, v2] + g[q] * dw
            B[v1, v2] += acc


def hessian(ob, atoms, coefficients):
    """(H, mixed, born) of the model (flat ``coefficients``) on one frame; ``ob`` an ``oracle.OracleBasis``."""
    c1, c2, c3 = O.split_coefficients(ob, coefficients)
    n = len(atoms.get_atomic_numbers())
    assert n <= 64
    s = ob.spec
    pair_rmax = np.asarray(ob.pair_rmax)
    rmin3 = rmax3 = 0.0
    tk = []
    off = 0
    for t in range(len(ob.trios)):
        ks = []
        for q in range(3):
            nk = int(ob.trio_nk[t][q])
            ks.append(ob.trio_knots[off:off + nk])
            off += nk
        tk.append(ks)
    if tk:
        rmin3 = min(k[0][0] for k in tk)
        rmax3 = max(max(k[0][-1], k[1][-1]) for k in tk)
    reach = max(pair_rmax.max(), rmax3)
    # a supercell wide enough for every image a real atom's terms reach (the reference's own range may drop some)
    sc_pos, sc_z, _ = O.supercell(atoms, 2.0 * reach)
    par = np.arange(len(sc_z)) % n
    zs = list(ob.species_z)
    pk, pc = [], []
    kp, cp = 0, 0
    for p in range(len(ob.pairs)):
        nk = int(ob.pair_nk[p])
        pk.append(ob.pair_knots[kp:kp + nk]); pc.append(c2[cp:cp + nk - 4])
        kp += nk; cp += nk - 4
    pair_of = {}
    for p, (za, zb) in enumerate(ob.pair_z):
        pair_of[(int(za), int(zb))] = p; pair_of[(int(zb), int(za))] = p
    trio_of = {}
    for t, (zc, za, zb) in enumerate(ob.trio_z):
        trio_of[(int(zc), int(za), int(zb))] = t
    grids, off = [], 0
    for t, shp in enumerate(ob.grid_shapes):
        size = int(np.prod(shp))
        grids.append(c3[off:off + size].reshape(shp)); off += size
    H = np.zeros((3 * n, 3 * n)); L = np.zeros((3 * n, 6)); B = np.zeros((6, 6))
    for i in range(n):
        d = sc_pos - sc_pos[i]
        r = np.linalg.norm(d, axis=1)
        zi = int(sc_z[i])
        for j in np.flatnonzero(r > 0):
            p = pair_of.get((zi, int(sc_z[j])))
            if p is None:
                continue
            rmin = max(float(ob.pair_rmin[p]), 0.0)
            if not (rmin < r[j] < pair_rmax[p]):
                continue
            g = float(pc[p] @ _basis(pk[p], r[j], 1)[0])
            k = float(pc[p] @ _basis(pk[p], r[j], 2)[0])
            _add(H, L, B, [i, par[j]], [(0, 1)], d[j][None], np.array([g]), np.array([[k]]))
        if not tk:
            continue
        nb = np.flatnonzero((r > rmin3) & (r <= rmax3))
        for x in range(len(nb)):
            for y in range(x + 1, len(nb)):
                j, k = nb[x], nb[y]
                if sc_z[j] > sc_z[k]:
                    j, k = k, j
                t = trio_of.get((zi, int(sc_z[j]), int(sc_z[k])))
                if t is None:
                    continue
                dv = np.array([d[j], d[k], d[k] - d[j]])
                rr = np.linalg.norm(dv, axis=1)
                if not all(tk[t][q][0] < rr[q] < tk[t][q][-1] for q in range(3)):
                    continue
                bv = [[_basis(tk[t][q], rr[q], nu)[0] for nu in range(3)] for q in range(3)]
                G = grids[t]

                def c(nl, nm, nn):
                    return float(np.einsum("abc,a,b,c->", G, bv[0][nl], bv[1][nm], bv[2][nn]))
                g = np.array([c(1, 0, 0), c(0, 1, 0), c(0, 0, 1)])
                K = np.array([[c(2, 0, 0), c(1, 1, 0), c(1, 0, 1)],
                              [c(1, 1, 0), c(0, 2, 0), c(0, 1, 1)],
                              [c(1, 0, 1), c(0, 1, 1), c(0, 0, 2)]])
                _add(H, L, B, [i, par[j], par[k]], [(0, 1), (0, 2), (1, 2)], dv, g, K)
    return H, L, B
