"""NumPy restatement of the phonon density of states and the harmonic thermodynamics (uf3_phonon_dos / uf3_phonon_thermo),
written from the formulas and not from the kernels: np.log1p / np.expm1 per mode, math.fsum for every sum.  Also the
dynamical matrix from a flat term list (``dynamical_from_terms``), the formula of the device's D(q) in a dozen lines."""
import math

import numpy as np

THZ = 15.633302
H = 4.135667696e-3        # eV / THz
KB = 8.617333262e-5       # eV / K


def dynamical_from_terms(fc_rows, terms, weights, q, masses):
    """D(q) [nq, 3N, 3N] from fc_rows [N, N_sc, 3, 3], terms [n, 5] = (i, p, n0, n1, n2) and their weights."""
    n = fc_rows.shape[0]
    q = np.atleast_2d(np.asarray(q, dtype=float))
    D = np.zeros((len(q), 3 * n, 3 * n), dtype=complex)
    phase = weights[None, :] * np.exp(2j * np.pi * (q @ terms[:, 2:].T.astype(float)))
    for k, (i, p) in enumerate(terms[:, :2]):
        j = p % n
        D[:, 3 * i:3 * i + 3, 3 * j:3 * j + 3] += phase[:, k, None, None] * fc_rows[i, p][None]
    s = np.repeat(1.0 / np.sqrt(np.asarray(masses, dtype=float)), 3)
    D *= s[None, :, None] * s[None, None, :]
    return 0.5 * (D + np.conj(np.transpose(D, (0, 2, 1))))


def frequencies(lam):
    lam = np.asarray(lam, dtype=float)
    return np.sign(lam) * np.sqrt(np.abs(lam)) * THZ


def smeared_dos(freqs, weights, samples, sigma):
    """g(f_s) = sum_q w_q sum_modes exp(-(f_s - f)^2 / 2 sigma^2) / (sigma sqrt(2 pi)) / sum_q w_q, every sum by math.fsum."""
    f = np.asarray(freqs, dtype=float)
    w = np.broadcast_to(np.asarray(weights, dtype=float)[:, None], f.shape).ravel()
    f = f.ravel()
    norm = sigma * math.sqrt(2.0 * math.pi) * math.fsum(np.asarray(weights, dtype=float))
    out = np.empty(len(samples))
    for k, fs in enumerate(np.asarray(samples, dtype=float)):
        z = (fs - f) / sigma
        out[k] = math.fsum(w * np.exp(-0.5 * z * z)) / norm
    return out


def mode_terms(f, T):
    """Per-mode F, U (eV), S, C_v (eV / K) of modes at frequencies f (THz, > 0) at temperature T (K)."""
    f = np.asarray(f, dtype=float)
    hf = H * f
    if T == 0:
        z = np.zeros_like(hf)
        return 0.5 * hf, 0.5 * hf, z, z
    kT = KB * T
    x = hf / kT
    with np.errstate(over="ignore"):
        l = np.log1p(-np.exp(-x))
        bose = 1.0 / np.expm1(x)
        cv = KB * x * x * np.exp(-x) / np.expm1(-x) ** 2          # = x^2 e^x / expm1(x)^2, without the overflow of e^x
    return 0.5 * hf + kT * l, hf * (0.5 + bose), KB * (x * bose - l), cv


def thermo(freqs, weights, temperatures, cutoff=1e-3, include=None):
    """dict of F, U, S, Cv [nT] per cell, their sums of absolute terms (``abs_F`` ...), ``zpe`` and ``n_excluded``.  Modes with
    f <= cutoff are left out -- or, with ``include`` (bool, like freqs), exactly the modes it names."""
    f = np.asarray(freqs, dtype=float)
    w = np.broadcast_to(np.asarray(weights, dtype=float)[:, None], f.shape)
    inc = f > cutoff if include is None else np.asarray(include, dtype=bool)
    wsum = math.fsum(np.asarray(weights, dtype=float))
    fi, wi = f[inc], w[inc]
    res = {k: [] for k in ("F", "U", "S", "Cv", "abs_F", "abs_U", "abs_S", "abs_Cv")}
    for T in temperatures:
        for name, term in zip(("F", "U", "S", "Cv"), mode_terms(fi, float(T))):
            res[name].append(math.fsum(wi * term) / wsum)
            res["abs_" + name].append(math.fsum(wi * np.abs(term)) / wsum)
        # F's two parts cancel near one temperature: its scale is the sum of both parts' magnitudes
        if T > 0:
            res["abs_F"][-1] = math.fsum(wi * (0.5 * H * fi + np.abs(mode_terms(fi, float(T))[0] - 0.5 * H * fi))) / wsum
    res = {k: np.array(v) for k, v in res.items()}
    res["zpe"] = math.fsum(wi * 0.5 * H * fi) / wsum
    res["n_excluded"] = int(round(math.fsum(w[~inc])))
    return res
