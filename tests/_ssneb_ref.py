"""NumPy restatement of the device nudged elastic band with changing cells (uf3_amd/csrc/uf3_neb.h, the cell instances): tests/_neb_ref.py's band
in tests/_relax_ref.py's generalised coordinates.  With C0 the cell of a band's first image, image i has D_i = C0^-1 C_i,
q_i = x_i D_i^-1 and the vector u_i = (q_i, Y_i = kappa D_i); its true force is (F D_i^T, -D_i^-T W_i / kappa).  Differences
between images as stored over all 3 n + 9 entries, the improved tangent, an optional climbing image, one FIRE per band, the
criterion the largest row norm of g (atom rows and cell rows).  Driven by an ``evaluate(positions, cells) -> (E, F, W)``
callback; records ``margins``, ``power`` and ``max_dr`` as tests/_neb_ref.py does.  For tests/test_ssneb_host.py and
tests/test_gpu_ssneb.py."""
import numpy as np

from _neb_ref import tangent
from _relax_ref import N_MIN, F_INC, F_DEC, A_START, F_A, RUNNING, CONVERGED, NONFINITE, voigt_to_matrix


def pack(q, Y):
    """u = (q [n, 3], Y [3, 3]) as one array [n + 3, 3]."""
    return np.concatenate([q, Y])


class CellBand:
    """``evaluate(positions [N, 3], cells [n_frames, 3, 3]) -> (energies [n_frames], forces [N, 3], W [n_frames, 6])``;
    ``offsets`` [n_frames + 1]; ``bands`` [n_bands + 1]: band b holds frames bands[b] .. bands[b + 1] - 1; ``spring`` and
    ``cell_factor`` a scalar or [n_bands] (``cell_factor`` None: the atom count of an image)."""

    def __init__(self, evaluate, positions, cells, offsets, bands, spring=0.1, cell_factor=None):
        self.evaluate = evaluate
        self.x = np.array(positions, dtype=float).reshape(-1, 3)
        self.cells = np.array(cells, dtype=float).reshape(-1, 3, 3)
        self.off = np.asarray(offsets, dtype=np.int64)
        self.bands = np.asarray(bands, dtype=np.int64)
        nb, nf = len(self.bands) - 1, len(self.off) - 1
        self.spring = np.broadcast_to(np.asarray(spring, dtype=float), (nb,)).copy()
        n_img = np.array([self.off[self.bands[b] + 1] - self.off[self.bands[b]] for b in range(nb)], dtype=float)
        self.kappa = n_img if cell_factor is None else np.broadcast_to(np.asarray(cell_factor, dtype=float), (nb,)).copy()
        self.D = np.zeros((nf, 3, 3))
        self.q = np.zeros_like(self.x)
        for b in range(nb):
            f0, f1 = self.bands[b], self.bands[b + 1]
            c0i = np.linalg.inv(self.cells[f0])
            for f in range(f0, f1):
                self.D[f] = np.eye(3) if f == f0 else c0i @ self.cells[f]
                lo, hi = self.off[f], self.off[f + 1]
                self.q[lo:hi] = self.x[lo:hi] @ np.linalg.inv(self.D[f])
        self.v = np.zeros_like(self.x)
        self.vc = np.zeros((nf, 3, 3))
        self.fq = np.zeros_like(self.x)             # the atom rows of the true force, F D^T, of the last evaluation
        self.G = np.zeros((nf, 3, 3))               # its cell part
        self.g = np.zeros_like(self.x)              # the atom rows of the NEB force of the last evaluation (0 on end points)
        self.gc = np.zeros((nf, 3, 3))              # its cell part
        self.dt = np.zeros(nb)
        self.alpha = np.full(nb, A_START)
        self.n_pos = np.zeros(nb, np.int64)
        self.first = np.ones(nb, bool)
        self.status = np.zeros(nb, np.int64)
        self.steps = np.zeros(nb, np.int64)
        self.crit = np.full(nb, np.nan)
        self.climbing = np.full(nb, -1, np.int64)
        self.e_last = np.full(nf, np.nan)
        self._forces = None
        self.margins = []            # per evaluation: the smallest margin of the comparisons of the bands that ran
        self.max_dr = 0.0            # the largest |dr| over a band's DOF (atoms and cells) in any step (tests: <= maxstep)
        self.power = []              # g.v / (|g| |v|) of every power test made

    def _span(self, b):
        f0, f1 = self.bands[b], self.bands[b + 1]
        return f0, f1 - f0, self.off[f0], self.off[f1]

    def true_force(self, b, F, W):
        """The generalised true force [M, n + 3, 3] of band b (None when a D is singular)."""
        f0, M, lo, hi = self._span(b)
        na = (hi - lo) // M
        out = np.zeros((M, na + 3, 3))
        for j in range(M):
            D = self.D[f0 + j]
            if not np.all(np.isfinite(D)) or np.linalg.det(D) == 0.0:
                return None
            out[j, :na] = F[lo + j * na:lo + (j + 1) * na] @ D.T
            out[j, na:] = -(np.linalg.inv(D).T @ voigt_to_matrix(W[f0 + j])) / self.kappa[b]
        return out

    def neb_force(self, b, e, FF, climb, margins=None):
        """(g [M, n + 3, 3], climbing image or -1, ok) of band b from its true force FF; ok False when a tangent vanishes."""
        f0, M, lo, hi = self._span(b)
        na = (hi - lo) // M
        U = np.array([pack(self.q[lo + j * na:lo + (j + 1) * na], self.kappa[b] * self.D[f0 + j]) for j in range(M)])
        E = e[f0:f0 + M]
        ci = -1
        if climb:
            ci = 1 + int(np.argmax(E[1:M - 1]))
            if margins is not None and M > 3:
                top = np.sort(E[1:M - 1])
                margins.append(top[-1] - top[-2])
        g = np.zeros((M, na + 3, 3))
        ok = True
        for i in range(1, M - 1):
            tp, tm = U[i + 1] - U[i], U[i] - U[i - 1]
            tau = tangent(tp, tm, E[i - 1], E[i], E[i + 1], margins)
            tn = np.sqrt(np.vdot(tau, tau))
            if not (tn > 0.0) or not np.isfinite(tn):
                ok = False
                continue
            that = tau / tn
            ft = np.vdot(FF[i], that)
            if i == ci:
                g[i] = FF[i] - 2.0 * ft * that
            else:
                g[i] = FF[i] - ft * that + self.spring[b] * (np.sqrt(np.vdot(tp, tp)) - np.sqrt(np.vdot(tm, tm))) * that
        return g, ci, ok

    def _band(self, b, e, F, W, fmax, climb, dt0, dt_max, maxstep, can_move, margins):
        f0, M, lo, hi = self._span(b)
        na = (hi - lo) // M
        self.e_last[f0:f0 + M] = e[f0:f0 + M]
        finite = np.all(np.isfinite(e[f0:f0 + M])) and np.all(np.isfinite(F[lo:hi])) and np.all(np.isfinite(W[f0:f0 + M]))
        ok = False
        if finite:
            FF = self.true_force(b, F, W)
            ok = FF is not None and np.all(np.isfinite(FF))
        if ok:
            g, ci, ok = self.neb_force(b, e, FF, climb, margins)
            ok = ok and np.all(np.isfinite(g))
        if not ok:
            self.status[b], self.crit[b], self.climbing[b] = NONFINITE, np.nan, -1
            return
        self.fq[lo:hi] = FF[:, :na].reshape(-1, 3)
        self.G[f0:f0 + M] = FF[:, na:]
        self.g[lo:hi] = g[:, :na].reshape(-1, 3)
        self.gc[f0:f0 + M] = g[:, na:]
        crit = np.sqrt((g * g).sum(-1)).max()                           # every row: atoms and cell
        self.crit[b], self.climbing[b] = crit, ci
        if crit < fmax:
            self.status[b] = CONVERGED
            return
        if not can_move:
            return
        g = g[1:M - 1]
        v = np.array([pack(self.v[lo + j * na:lo + (j + 1) * na], self.vc[f0 + j]) for j in range(1, M - 1)])
        dt = dt0 if self.first[b] else self.dt[b]
        if not self.first[b]:
            scale = np.sqrt(np.vdot(g, g) * np.vdot(v, v))
            self.power.append(np.vdot(g, v) / scale if scale > 0 else 0.0)
            if np.vdot(g, v) > 0:
                v = (1 - self.alpha[b]) * v + self.alpha[b] * np.sqrt(np.vdot(v, v)) / np.sqrt(np.vdot(g, g)) * g
                if self.n_pos[b] > N_MIN:
                    dt = min(dt * F_INC, dt_max)
                    self.alpha[b] *= F_A
                self.n_pos[b] += 1
            else:
                v = 0.0 * v
                self.alpha[b], dt, self.n_pos[b] = A_START, dt * F_DEC, 0
        v = v + dt * g
        dr = dt * v
        norm = np.sqrt(np.vdot(dr, dr))
        if norm > maxstep:
            dr = dr * (maxstep / norm)
        self.max_dr = max(self.max_dr, float(np.sqrt(np.vdot(dr, dr))))
        for j in range(1, M - 1):
            f, a, z = f0 + j, lo + j * na, lo + (j + 1) * na
            self.v[a:z], self.vc[f] = v[j - 1, :na], v[j - 1, na:]
            self.q[a:z] += dr[j - 1, :na]
            self.D[f] = self.D[f] + dr[j - 1, na:] / self.kappa[b]
            self.x[a:z] = self.q[a:z] @ self.D[f]
            self.cells[f] = self.cells[f0] @ self.D[f]
        self.dt[b] = dt
        self.first[b] = False
        self.steps[b] += 1

    def run(self, max_steps, fmax=0.05, climb=False, dt=0.1, dt_max=1.0, maxstep=0.2):
        """Evaluations 0 .. max_steps; each but the last moves the bands still running.  Returns the energies of every
        evaluation.  A band that converged in an earlier run is tested again; a frozen band stays frozen."""
        self.status[self.status == CONVERGED] = RUNNING
        energies = []
        for k in range(max_steps + 1):
            if not (k == 0 and self._forces is not None):
                self._forces = self.evaluate(self.x, self.cells)
                fresh = True
            else:
                fresh = False
            e, F, W = self._forces
            margins = []
            for b in range(len(self.bands) - 1):
                if self.status[b] == RUNNING:
                    self._band(b, e, F, W, fmax, climb, dt, dt_max, maxstep, k < max_steps, margins)
            if fresh or not self.margins:
                self.margins.append(min(margins) if margins else np.inf)
            else:
                self.margins[-1] = min([self.margins[-1]] + margins)
            energies.append(self.e_last.copy())
            if k < max_steps and np.any(self.status == RUNNING):
                self._forces = None
            if not np.any(self.status == RUNNING):
                break
        return np.array(energies)


class MorsePair:
    """An analytic periodic pair potential for host tests: phi(r) = eps (e^{-2 a (r - r0)} - 2 e^{-a (r - r0)}) (1 - (r / rc)^2)^2
    for r < rc, summed over every image within ``reach`` cells along each axis.  ``__call__(positions, cells)`` returns
    (energies [n_frames], forces [N, 3], dE/d(strain) [n_frames, 6] in Voigt order xx, yy, zz, yz, xz, xy)."""

    def __init__(self, offsets, eps=0.4, a=1.3, r0=2.75, rc=4.6, reach=3):
        self.off = np.asarray(offsets, dtype=np.int64)
        self.eps, self.a, self.r0, self.rc = eps, a, r0, rc
        k = np.arange(-reach, reach + 1)
        self.shifts = np.array(np.meshgrid(k, k, k, indexing="ij")).reshape(3, -1).T.astype(float)

    def frame(self, x, cell):
        d = x[None, :, None, :] - x[:, None, None, :] + (self.shifts @ cell)[None, None]       # [i, j, image, 3]: x_j + T - x_i
        r = np.sqrt((d * d).sum(-1))
        ok = (r > 1e-9) & (r < self.rc)
        rs = np.where(ok, r, 1.0)
        ex = np.exp(-self.a * (rs - self.r0))
        m, dm = self.eps * (ex * ex - 2 * ex), self.eps * (-2 * self.a * ex * ex + 2 * self.a * ex)
        u = 1 - (rs / self.rc) ** 2
        s, ds = u * u, -4 * u * rs / self.rc ** 2
        phi = np.where(ok, m * s, 0.0)
        dphi = np.where(ok, dm * s + m * ds, 0.0)
        w = dphi / rs                                                                           # phi' / r
        e = 0.5 * phi.sum()
        f = (w[..., None] * d).sum((1, 2))                                                      # -dE/dx_i
        W = 0.5 * np.einsum("ijk,ijka,ijkb->ab", w, d, d)
        return e, f, np.array([W[0, 0], W[1, 1], W[2, 2], W[1, 2], W[0, 2], W[0, 1]])

    def __call__(self, positions, cells):
        nf = len(self.off) - 1
        e, F, W = np.zeros(nf), np.zeros_like(positions), np.zeros((nf, 6))
        for f in range(nf):
            lo, hi = self.off[f], self.off[f + 1]
            e[f], F[lo:hi], W[f] = self.frame(positions[lo:hi], np.asarray(cells[f], dtype=float).reshape(3, 3))
        return e, F, W
