"""NumPy restatement of the switching scheme of uf3_amd/csrc/uf3_ti.h (``uf3_md_run_switch``): molecular dynamics on
H(lambda) = K + lambda U + (1 - lambda) U_E with a per-frame lambda and temperature, the work accumulated by the trapezoid
rule, force and noise projected when the centre of mass is held.  Built on tests/_md_ref.py's generator; for
tests/test_ti_host.py and tests/test_gpu_ti.py."""
import numpy as np

from uf3_amd.forcefield.md import ACC, KB, KE_UNIT
from _md_ref import normals3


def run_switch(x, v, masses, forces_of, offsets, x0, k, n_steps, dt, temperatures, friction, seed, lam_a, lam_b, schedule,
               fix_com, step0=0, every=0):
    """``n_steps`` steps from (x, v); forces_of(x) -> (energies [n_frames], forces [N, 3]); offsets [n_frames + 1]; x0 [N, 3]
    and k [N] the Einstein crystal; temperatures, lam_a, lam_b [n_frames]; schedule [n_steps + 1].  Returns x, v, the work
    [n_frames] and the records [n_steps // every, n_frames, 5] = [lambda, U, U_E, KE, W so far]."""
    x, v = np.array(x, dtype=float), np.array(v, dtype=float)
    m, k = np.asarray(masses, dtype=float), np.asarray(k, dtype=float)
    offsets = np.asarray(offsets, dtype=np.int64)
    n_frames = len(offsets) - 1
    frame_of = np.repeat(np.arange(n_frames), np.diff(offsets))
    lam_a, lam_b = (np.broadcast_to(np.asarray(a, dtype=float), (n_frames,)) for a in (lam_a, lam_b))
    kt = KB * np.broadcast_to(np.asarray(temperatures, dtype=float), (n_frames,))
    ka = (ACC / m)[:, None]

    def per_frame(a):
        return np.add.reduceat(a, offsets[:-1], axis=0)

    total_mass = per_frame(m)

    def state(j):
        e, f = forces_of(x)
        lam = lam_a + (lam_b - lam_a) * schedule[j]
        d = x - x0
        u_e = per_frame(0.5 * k * np.sum(d * d, axis=1))
        la = lam[frame_of, None]
        force = la * f - (1.0 - la) * k[:, None] * d
        if fix_com:
            force = force - m[:, None] * (per_frame(force) / total_mass[:, None])[frame_of]
        return np.asarray(e, dtype=float), u_e, lam, force

    c = np.exp(-friction * dt)
    e, u_e, lam, force = state(0)
    work, records = np.zeros(n_frames), []
    for j in range(n_steps):
        v = v + 0.5 * dt * force * ka
        if friction > 0:
            x = x + 0.5 * dt * v
            dv = np.sqrt((1 - c * c) * kt[frame_of, None] * ka) * normals3(seed, np.arange(len(x)), step0 + j, 0)
            if fix_com:
                dv = dv - (per_frame(m[:, None] * dv) / total_mass[:, None])[frame_of]
            v = c * v + dv
            x = x + 0.5 * dt * v
        else:
            x = x + dt * v
        d_before, lam_before = e - u_e, lam
        e, u_e, lam, force = state(j + 1)
        work = work + (lam - lam_before) * 0.5 * (d_before + (e - u_e))
        v = v + 0.5 * dt * force * ka
        if every and (j + 1) % every == 0:
            ke = 0.5 * per_frame(m * np.sum(v * v, axis=1)) * KE_UNIT
            records.append(np.stack([lam, e, u_e, ke, work], axis=1))
    return x, v, work, np.array(records).reshape(len(records), n_frames, 5)


def constrained_logdet(matrix, masses):
    """log det(Q^T matrix Q) of a [3N, 3N] matrix, Q an orthonormal basis of the displacements with sum_i m_i u_i = 0."""
    m = np.asarray(masses, dtype=float)
    con = np.zeros((3, 3 * len(m)))
    for d in range(3):
        con[d, d::3] = m
    q = np.linalg.svd(con)[2][3:].T
    sign, logdet = np.linalg.slogdet(q.T @ matrix @ q)
    assert sign > 0
    return logdet
