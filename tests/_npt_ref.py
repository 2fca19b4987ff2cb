"""NumPy restatement of the constant-pressure integrator (uf3_amd/csrc/uf3_npt.h): isotropic
Martyna-Tobias-Klein dynamics, every frame its own piston, for tests/test_npt_host.py and tests/test_gpu_npt.py.

A frame's cell is s * cell0, v_eps = d ln s / dt (1/fs), N_f = 3N, alpha = 1 + 1/N, W_p = (3N + 3) k_B T_p tau_p^2:

    dr/dt = v + v_eps r     dv/dt = F/m - alpha v_eps v     ds/dt = v_eps s
    W_p dv_eps/dt = G = alpha tr K - tr W - 3 P0 V          (K = sum m v (x) v, W = dE/d(strain), eV)

One step, h = dt / 2, every sub-step the exact solution of its own sub-equation:

    P  v_eps += h G / W_p
    B  v = a v + b F/m,   a = exp(-x), b = h (1 - exp(-x)) / x, x = alpha v_eps h
    A  r = e r + d v, s = e s,   e = exp(v_eps dt), d = dt (e - 1) / (v_eps dt)
       (with a thermostat: A(h); O on the atoms: v = c v + sqrt((1 - c^2) k_B T / m) xi; O on the piston:
        v_eps = c_p v_eps + sqrt((1 - c_p^2) k_B T / W_p) xi_p; A(h) with the new v_eps)
    -- energy, forces, tr W at the new positions and cell --
    B, P

``evaluate(x, scales)`` -> (energies [n_frames], forces [N, 3], tr W [n_frames]).  The piston of frame f draws the first
normal of Philox counter (2^31 | f, step lo, step hi, 0); the atoms draw as in tests/_md_ref.py."""
import numpy as np

from uf3_amd.forcefield.md import ACC, KB, KE_UNIT
from _md_ref import normals3


def phi(x):
    """(1 - exp(-x)) / x"""
    x = np.asarray(x, dtype=float)
    small = np.abs(x) < 1e-4
    xs = np.where(small, 1.0, x)
    return np.where(small, 1.0 - x * (0.5 - x * (1.0 / 6.0 - x * (1.0 / 24.0))), -np.expm1(-xs) / xs)


def psi(x):
    """(exp(x) - 1) / x"""
    x = np.asarray(x, dtype=float)
    small = np.abs(x) < 1e-4
    xs = np.where(small, 1.0, x)
    return np.where(small, 1.0 + x * (0.5 + x * (1.0 / 6.0 + x * (1.0 / 24.0))), np.expm1(xs) / xs)


class Pistons:
    """Per-frame bookkeeping: frame of every atom, N, alpha, W_p, V0."""

    def __init__(self, offsets, volumes0, tau_fs, piston_temperature_K):
        self.off = np.asarray(offsets, dtype=np.int64)
        self.n = np.diff(self.off).astype(float)
        self.frame_of = np.repeat(np.arange(len(self.n)), np.diff(self.off))
        self.alpha = 1.0 + 1.0 / self.n
        self.wp = (3.0 * self.n + 3.0) * KB * piston_temperature_K * tau_fs ** 2
        self.vol0 = np.asarray(volumes0, dtype=float)

    def tr_k(self, v, masses):
        return KE_UNIT * np.add.reduceat(masses * np.sum(v * v, axis=1), self.off[:-1])

    def g(self, v, masses, tr_w, s, p0):
        return self.alpha * self.tr_k(v, masses) - tr_w - 3.0 * p0 * self.vol0 * s ** 3

    def conserved(self, v, masses, e, s, veps, p0):
        return 0.5 * self.tr_k(v, masses) + e + p0 * self.vol0 * s ** 3 + 0.5 * self.wp * veps ** 2


def run(x, v, masses, pistons, s, veps, evaluate, n_steps, dt, p0, temperature_K=0.0, friction=0.0, barostat_friction=0.0, seed=0,
        step0=0, history=False):
    """``n_steps`` constant-pressure steps.  Returns x, v, s, veps, energies, forces (and, with ``history``, the conserved
    quantity [n_steps + 1, n_frames] at every integer time)."""
    P = pistons
    x, v = np.array(x, dtype=float), np.array(v, dtype=float)
    s, veps = np.array(s, dtype=float), np.array(veps, dtype=float)
    ka = (ACC / masses)[:, None]
    fo = P.frame_of
    h = 0.5 * dt
    langevin = friction > 0 or barostat_friction > 0
    c, cp = np.exp(-friction * dt), np.exp(-barostat_friction * dt)
    kT = KB * temperature_K
    e, f, tr_w = evaluate(x, s)
    g = P.g(v, masses, tr_w, s, p0)
    hist = [P.conserved(v, masses, e, s, veps, p0)]
    for k in range(n_steps):
        veps = veps + h * g / P.wp
        xk = P.alpha * veps * h
        a2, b2 = np.exp(-xk), h * phi(xk)
        v = a2[fo, None] * v + b2[fo, None] * (f * ka)
        if langevin:
            y1 = veps * h
            e1, d1 = np.exp(y1), h * psi(y1)
            x = e1[fo, None] * x + d1[fo, None] * v
            xi = normals3(seed, np.arange(len(x)), step0 + k, 0)
            v = c * v + np.sqrt((1 - c * c) * kT * ka) * xi
            xi_p = normals3(seed, (1 << 31) | np.arange(len(s), dtype=np.int64), step0 + k, 0)[:, 0]
            veps = cp * veps + np.sqrt((1 - cp * cp) * kT / P.wp) * xi_p
            y2 = veps * h
            e2, d2 = np.exp(y2), h * psi(y2)
            x = e2[fo, None] * x + d2[fo, None] * v
            s = s * e1
            s = s * e2
        else:
            y = veps * dt
            e1, d1 = np.exp(y), dt * psi(y)
            x = e1[fo, None] * x + d1[fo, None] * v
            s = s * e1
        e, f, tr_w = evaluate(x, s)
        xk = P.alpha * veps * h
        a1, b1 = np.exp(-xk), h * phi(xk)
        v = a1[fo, None] * v + b1[fo, None] * (f * ka)
        g = P.g(v, masses, tr_w, s, p0)
        veps = veps + h * g / P.wp
        hist.append(P.conserved(v, masses, e, s, veps, p0))
    out = (x, v, s, veps, e, f)
    return out + (np.array(hist),) if history else out
