"""NumPy restatement of what the eigenvector routes compute (uf3_phonon_mesh_vec / _pdos / _tdisp), written from the formulas and
not from the kernels: dD / dq from the term records, Hellmann-Feynman group velocities from given vectors and their sums over
degenerate clusters, the projected smeared DOS and the thermal displacement tensors (math.fsum for every sum over modes)."""
import math

import numpy as np

import _phonon_ref as PR

VOIGT = ((0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1))


def unit_phase(x):
    """exp(2 pi i x) with the argument folded first: x mod 1 into [-1/2, 1/2], then sine and cosine of pi y (y = 2x) from the
    nearest of 0, 1/2, 1 -- exact at the quarter turns.  np.exp(2j pi x) leaves sin(pi k) ~ 1e-16 k at half-integer x, which is
    all there is of dD / dq at the time-reversal-invariant points, where dD / dq vanishes."""
    x = np.asarray(x, dtype=float)
    y = 2.0 * (x - np.round(x))
    a = np.abs(y)
    mid = (a > 0.25) & (a <= 0.75)
    far = a > 0.75
    s = np.where(mid, np.cos(np.pi * (0.5 - a)), np.where(far, np.sin(np.pi * (1.0 - a)), np.sin(np.pi * a))) * np.sign(y)
    c = np.where(mid, np.sin(np.pi * (0.5 - a)), np.where(far, -np.cos(np.pi * (1.0 - a)), np.cos(np.pi * a)))
    return c + 1j * s


def d_dynamical_from_terms(fc_rows, terms, weights, q, masses):
    """dD / dq_a [nq, 3, 3N, 3N]: ``_phonon_ref.dynamical_from_terms`` with the factor 2 pi i n_a on every term (and the phases
    by ``unit_phase``)."""
    n = fc_rows.shape[0]
    q = np.atleast_2d(np.asarray(q, dtype=float))
    lat = terms[:, 2:].astype(float)
    phase = weights[None, :] * unit_phase(q @ lat.T)
    dD = np.zeros((len(q), 3, 3 * n, 3 * n), dtype=complex)
    for k, (i, p) in enumerate(terms[:, :2]):
        j = p % n
        fac = 2j * np.pi * lat[k][None, :] * phase[:, k, None]                      # [nq, 3]
        dD[:, :, 3 * i:3 * i + 3, 3 * j:3 * j + 3] += fac[:, :, None, None] * fc_rows[i, p][None, None]
    s = np.repeat(1.0 / np.sqrt(np.asarray(masses, dtype=float)), 3)
    dD *= s[None, None, :, None] * s[None, None, None, :]
    return 0.5 * (dD + np.conj(np.transpose(dD, (0, 1, 3, 2))))


def d_dynamical_dk(dD, cell):
    """dD / dk_c [nq, 3, 3N, 3N], k the Cartesian wave vector without 2 pi: q_a = sum_c k_c cell[a][c]."""
    return np.einsum("qaij,ac->qcij", dD, np.asarray(cell, dtype=float).reshape(3, 3))


def velocities(dD, vec, lam, cell, cutoff=1e-3):
    """v [nq, 3N, 3] (THz A) = THZ (v_s^H dD/dk_c v_s) / (2 sqrt|lam_s|); 0 where |f_s| <= cutoff."""
    dk = d_dynamical_dk(dD, cell)
    g = np.einsum("qis,qcij,qjs->qsc", np.conj(vec), dk, vec).real
    lam = np.asarray(lam, dtype=float)
    keep = np.abs(PR.frequencies(lam)) > cutoff
    with np.errstate(divide="ignore", invalid="ignore"):
        v = PR.THZ * g / (2.0 * np.sqrt(np.abs(lam)))[:, :, None]
    return np.where(keep[:, :, None], v, 0.0)


def velocity_scale(dD, lam, cell):
    """|dD / dk|_F THZ / (2 sqrt|lam_s|) [nq, 3N]: what a relative bound on the velocities is relative to."""
    dk = d_dynamical_dk(dD, cell)
    norm = np.sqrt((np.abs(dk) ** 2).sum(axis=(1, 2, 3)))
    with np.errstate(divide="ignore"):
        return norm[:, None] * PR.THZ / (2.0 * np.sqrt(np.abs(np.asarray(lam, dtype=float))))


def clusters(lam_row, rel_gap=1e-6):
    """Index lists of the degenerate clusters of one ascending row of eigenvalues: a new cluster where the gap to the previous
    eigenvalue exceeds rel_gap max|lam|."""
    lam_row = np.asarray(lam_row, dtype=float)
    cut = np.flatnonzero(np.diff(lam_row) > rel_gap * np.abs(lam_row).max()) + 1
    return [list(c) for c in np.split(np.arange(len(lam_row)), cut)]


def cluster_sums(v_row, groups):
    return np.array([v_row[g].sum(axis=0) for g in groups])


def projected_dos(freqs, vec, weights, samples, sigma):
    """g_c(f) [3N, n_samples] = sum_q w_q sum_s |V_cs|^2 exp(-(f - f_s)^2 / 2 sigma^2) / (sigma sqrt(2 pi)) / sum_q w_q."""
    f = np.asarray(freqs, dtype=float)
    nq, n3 = f.shape
    w = np.asarray(weights, dtype=float)
    p = (np.abs(vec) ** 2) * w[:, None, None]                                       # [nq, channel, mode]
    norm = sigma * math.sqrt(2.0 * math.pi) * math.fsum(w)
    out = np.empty((n3, len(samples)))
    for k, fs in enumerate(np.asarray(samples, dtype=float)):
        z = (fs - f) / sigma
        gk = np.exp(-0.5 * z * z)                                                   # [nq, mode]
        for c in range(n3):
            out[c, k] = math.fsum((p[:, c, :] * gk).ravel()) / norm
    return out


def displacement_tensors(lam, vec, weights, masses, temperatures, cutoff=1e-3):
    """(U6 [nT, N, 6], abs6 [nT, N, 6] the sums of the absolute terms, n_excluded): U_i^{ab} = (1 / sum w) sum_q w_q sum_s
    E_s / (m_i lam_s) Re(V_{3i+a,s} conj V_{3i+b,s}) over the modes with f > cutoff, E_s ``_phonon_ref.mode_terms``'s U."""
    lam = np.asarray(lam, dtype=float)
    f = PR.frequencies(lam)
    w = np.broadcast_to(np.asarray(weights, dtype=float)[:, None], f.shape)
    inc = f > cutoff
    wsum = math.fsum(np.asarray(weights, dtype=float))
    n = lam.shape[1] // 3
    U = np.zeros((len(temperatures), n, 6))
    A = np.zeros_like(U)
    for it, T in enumerate(temperatures):
        e = np.zeros_like(f)
        e[inc] = PR.mode_terms(f[inc], float(T))[1]
        with np.errstate(divide="ignore", invalid="ignore"):
            coef = np.where(inc, w * e / lam, 0.0)                                  # [nq, mode]
        for i in range(n):
            for k, (a, b) in enumerate(VOIGT):
                t = coef * (vec[:, 3 * i + a, :] * np.conj(vec[:, 3 * i + b, :])).real / masses[i]
                U[it, i, k] = math.fsum(t.ravel()) / wsum
                A[it, i, k] = math.fsum(np.abs(t).ravel()) / wsum
    return U, A, int(round(math.fsum(w[~inc])))
