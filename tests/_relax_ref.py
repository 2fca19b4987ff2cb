"""NumPy restatement of the device relaxation (uf3_amd/csrc/uf3_relax.h): per-frame FIRE in ASE's formulation with optional
cell degrees of freedom (x = q D, cell = cell0 D, cell coordinates n D, force on them -D^-T W / n) and fixed atoms, driven by a
force / strain-derivative callback.  For tests/test_relax_host.py and tests/test_gpu_relax.py."""
import numpy as np

N_MIN, F_INC, F_DEC, A_START, F_A = 5, 1.1, 0.5, 0.1, 0.99
RUNNING, CONVERGED, NONFINITE = 0, 1, 2


def voigt_to_matrix(w):
    """dE/d(strain) in Voigt order (xx, yy, zz, yz, xz, xy) -> the symmetric 3x3 matrix."""
    return np.array([[w[0], w[5], w[4]], [w[5], w[1], w[3]], [w[4], w[3], w[2]]])


def cell_force(D, W, n):
    """Force on the cell coordinates Y = n D: -D^-T W / n."""
    return -(np.linalg.inv(D).T @ W) / n


class Fire:
    """``evaluate(positions [N, 3], cells [nf, 3, 3]) -> (energies [nf], forces [N, 3], W [nf, 6] or None)``."""

    def __init__(self, evaluate, positions, cells, pbc, offsets, relax_cell=False, fixed=None):
        self.evaluate = evaluate
        self.x = np.array(positions, dtype=float).reshape(-1, 3)
        self.cells = np.array(cells, dtype=float).reshape(-1, 3, 3)
        self.off = np.asarray(offsets, dtype=np.int64)
        nf = len(self.off) - 1
        pbc = np.asarray(pbc, dtype=bool).reshape(nf, 3)
        if fixed is not None and relax_cell:
            raise ValueError("fixed atoms together with relax_cell")
        self.fixed = np.zeros(len(self.x), bool) if fixed is None else np.asarray(fixed, bool).copy()
        self.cellf = np.array([relax_cell and bool(p.all()) for p in pbc])
        self.cell0 = self.cells.copy()
        self.q = self.x.copy()
        self.D = np.array([np.eye(3) for _ in range(nf)])
        self.v = np.zeros_like(self.x)
        self.vc = np.zeros((nf, 3, 3))
        self.dt = np.zeros(nf)
        self.alpha = np.full(nf, A_START)
        self.n_pos = np.zeros(nf, np.int64)
        self.first = np.ones(nf, bool)
        self.status = np.zeros(nf, np.int64)
        self.steps = np.zeros(nf, np.int64)
        self.e_last = np.full(nf, np.nan)
        self.fmax_last = np.full(nf, np.nan)
        self._forces = None
        self.max_dr = 0.0            # the largest |dr| over a frame's DOF in any step (tests: <= maxstep)
        self.first_dt = []           # (frame, dt of its first move)
        self.power = []              # P / (|g| |v|) of every power test made: how far from 0 the branch was decided

    def _eval(self):
        self._forces = self.evaluate(self.x, self.cells)

    def _frame(self, f, e, F, W, fmax, dt0, dt_max, maxstep, can_move):
        lo, hi = self.off[f], self.off[f + 1]
        n = hi - lo
        Ff = F[lo:hi]
        fixed = self.fixed[lo:hi]
        G = np.zeros((3, 3))
        finite = np.isfinite(e) and np.all(np.isfinite(Ff))
        if self.cellf[f]:
            Wm = voigt_to_matrix(W[f])
            finite = finite and np.all(np.isfinite(Wm))
            if finite:
                G = cell_force(self.D[f], Wm, n)
        crit = np.nan
        if finite:
            free = np.where(fixed[:, None], 0.0, Ff)
            crit = max(np.sqrt((free * free).sum(1)).max(), np.sqrt((G * G).sum(1)).max())
        self.e_last[f], self.fmax_last[f] = e, crit
        if not finite:
            self.status[f] = NONFINITE
            return
        if crit < fmax:
            self.status[f] = CONVERGED
            return
        if not can_move:
            return
        g = Ff @ self.D[f].T if self.cellf[f] else Ff.copy()
        g[fixed] = 0.0
        v, vc = self.v[lo:hi], self.vc[f]
        dt = dt0 if self.first[f] else self.dt[f]
        if self.first[f]:
            self.first_dt.append((f, dt))
        else:
            P = np.vdot(g, v) + np.vdot(G, vc)
            scale = np.sqrt((np.vdot(g, g) + np.vdot(G, G)) * (np.vdot(v, v) + np.vdot(vc, vc)))
            self.power.append(P / scale if scale > 0 else 0.0)
            if P > 0:
                vn = np.sqrt(np.vdot(v, v) + np.vdot(vc, vc))
                gn = np.sqrt(np.vdot(g, g) + np.vdot(G, G))
                c = self.alpha[f] * vn / gn
                v = (1 - self.alpha[f]) * v + c * g
                vc = (1 - self.alpha[f]) * vc + c * G
                if self.n_pos[f] > N_MIN:
                    dt = min(dt * F_INC, dt_max)
                    self.alpha[f] *= F_A
                self.n_pos[f] += 1
            else:
                v, vc = 0.0 * v, 0.0 * vc
                self.alpha[f], dt, self.n_pos[f] = A_START, dt * F_DEC, 0
        v = v + dt * g
        vc = vc + dt * G
        dr, drc = dt * v, dt * vc
        norm = np.sqrt(np.vdot(dr, dr) + np.vdot(drc, drc))
        if norm > maxstep:
            dr, drc = dr * (maxstep / norm), drc * (maxstep / norm)
        self.max_dr = max(self.max_dr, float(np.sqrt(np.vdot(dr, dr) + np.vdot(drc, drc))))
        v[fixed] = 0.0
        dr[fixed] = 0.0
        self.v[lo:hi], self.vc[f] = v, vc
        if self.cellf[f]:
            self.q[lo:hi] += dr
            self.D[f] = self.D[f] + drc / n
            self.cells[f] = self.cell0[f] @ self.D[f]
            self.x[lo:hi] = self.q[lo:hi] @ self.D[f]
        else:
            self.x[lo:hi] += dr
        self.dt[f] = dt
        self.first[f] = False
        self.steps[f] += 1

    def run(self, max_steps, fmax=0.05, dt=0.1, dt_max=1.0, maxstep=0.2):
        """Evaluations 0 .. max_steps; each but the last moves the frames still running.  Returns the energies of every
        evaluation [max_steps + 1 or fewer, nf] (the loop stops once no frame runs)."""
        energies = []
        for k in range(max_steps + 1):
            if not (k == 0 and self._forces is not None):
                self._eval()
            e, F, W = self._forces
            for f in range(len(self.off) - 1):
                if self.status[f] == RUNNING:
                    self._frame(f, e[f], F, W, fmax, dt, dt_max, maxstep, k < max_steps)
            energies.append(self.e_last.copy())
            if k < max_steps and np.any(self.status == RUNNING):
                self._forces = None
            if not np.any(self.status == RUNNING):
                break
        return np.array(energies)
