"""NumPy restatement of the device integrator (uf3_amd/csrc/uf3_md.h): Philox4x32-10, its normals, Maxwell-Boltzmann
initialisation and the velocity Verlet / BAOAB step, for tests/test_md_host.py and tests/test_gpu_md.py."""
import numpy as np

from uf3_amd.forcefield.md import ACC, KB, KE_UNIT

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = np.uint32(0x9E3779B9), np.uint32(0xBB67AE85)
_LO = np.uint64(0xFFFFFFFF)


def philox(counters, keys):
    """Philox4x32-10 (Salmon et al., SC'11): counters [n, 4], keys [n, 2] (uint32) -> [n, 4] uint32."""
    ctr = np.asarray(counters, dtype=np.uint32).reshape(-1, 4)
    key = np.broadcast_to(np.asarray(keys, dtype=np.uint32).reshape(-1, 2), (len(ctr), 2))
    x0, x1, x2, x3 = (ctr[:, i].astype(np.uint64) for i in range(4))
    k0, k1 = key[:, 0].copy(), key[:, 1].copy()
    for _ in range(10):
        p0, p1 = _M0 * x0, _M1 * x2
        x0, x1, x2, x3 = (p1 >> np.uint64(32)) ^ x1 ^ k0.astype(np.uint64), p1 & _LO, (p0 >> np.uint64(32)) ^ x3 ^ k1.astype(np.uint64), p0 & _LO
        k0, k1 = k0 + _W0, k1 + _W1
    return np.stack([x0, x1, x2, x3], 1).astype(np.uint32)


def _uniform(hi, lo):
    u = (hi.astype(np.uint64) << np.uint64(32)) | lo.astype(np.uint64)
    return ((u >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53


def normals3(seed, atoms, step, draw):
    """[n, 3] normals of atoms ``atoms`` (global indices) in the step opened at absolute ``step``: draws ``draw``, ``draw + 1``."""
    atoms = np.asarray(atoms, dtype=np.int64)
    key = np.array([seed & 0xFFFFFFFF, seed >> 32], dtype=np.uint64).astype(np.uint32)
    out = []
    for d in (draw, draw + 1):
        ctr = np.zeros((len(atoms), 4), dtype=np.uint32)
        ctr[:, 0] = atoms.astype(np.uint32)
        ctr[:, 1] = step & 0xFFFFFFFF
        ctr[:, 2] = step >> 32
        ctr[:, 3] = d
        r = philox(ctr, key)
        rad = np.sqrt(-2.0 * np.log(_uniform(r[:, 0], r[:, 1])))
        phi = 2.0 * np.pi * _uniform(r[:, 2], r[:, 3])
        out.append(np.stack([rad * np.cos(phi), rad * np.sin(phi)], 1))
    return np.concatenate([out[0], out[1][:, :1]], 1)


def init_velocities(masses, offsets, temperature_K, seed, step, exact=False):
    n = len(masses)
    v = np.sqrt(KB * temperature_K / masses * ACC)[:, None] * normals3(seed, np.arange(n), step, 2)
    for lo, hi in zip(offsets[:-1], offsets[1:]):
        m = masses[lo:hi, None]
        v[lo:hi] -= (m * v[lo:hi]).sum(0) / m.sum()
        if exact:
            ke = 0.5 * float((m * v[lo:hi] ** 2).sum()) * KE_UNIT
            if ke > 0:
                v[lo:hi] *= np.sqrt(KB * temperature_K * 1.5 * (hi - lo) / ke)
    return v


def run(x, v, masses, forces_of, n_steps, dt, temperature_K=0.0, friction=0.0, seed=0, step0=0):
    """``n_steps`` of velocity Verlet (friction 0) or BAOAB; forces_of(x) -> (energies, forces).  Returns x, v, energies, forces."""
    x, v = np.array(x, dtype=float), np.array(v, dtype=float)
    ka = (ACC / masses)[:, None]
    e, f = forces_of(x)
    c = np.exp(-friction * dt)
    for k in range(n_steps):
        v = v + 0.5 * dt * f * ka
        if friction > 0:
            x = x + 0.5 * dt * v
            xi = normals3(seed, np.arange(len(x)), step0 + k, 0)
            v = c * v + np.sqrt((1 - c * c) * KB * temperature_K * ka) * xi
            x = x + 0.5 * dt * v
        else:
            x = x + dt * v
        e, f = forces_of(x)
        v = v + 0.5 * dt * f * ka
    return x, v, e, f
