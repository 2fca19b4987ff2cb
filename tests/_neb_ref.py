"""NumPy restatement of the device nudged elastic band (uf3_amd/csrc/uf3_neb.h): bands of consecutive frames with fixed end
points, the improved tangent (Henkelman & Jonsson 2000), an optional climbing image, differences between images as stored, and
one FIRE (tests/_relax_ref.py's constants and rules) per band over all its interior images, driven by an energy / force
callback.  Every evaluation also leaves the smallest margin of the energy comparisons it branched on (``margins``).  For
tests/test_neb_host.py and tests/test_gpu_neb.py."""
import numpy as np

from _relax_ref import N_MIN, F_INC, F_DEC, A_START, F_A, RUNNING, CONVERGED, NONFINITE


def tangent(tp, tm, em, e0, ep, margins=None):
    """The improved tangent (not normalised) of an image from t+ = R_{i+1} - R_i, t- = R_i - R_{i-1} and the three energies.
    ``margins``: a list that receives the margin of every comparison made."""
    dp, dm = abs(ep - e0), abs(em - e0)
    if margins is not None:
        margins += [dp, dm]
    if ep > e0 > em:
        return tp.copy()
    if ep < e0 < em:
        return tm.copy()
    dmax, dmin = max(dp, dm), min(dp, dm)
    if margins is not None:
        margins.append(abs(ep - em))
    return tp * dmax + tm * dmin if ep > em else tp * dmin + tm * dmax


class Band:
    """``evaluate(positions [N, 3]) -> (energies [n_frames], forces [N, 3])``; ``offsets`` [n_frames + 1]; ``bands``
    [n_bands + 1]: band b holds frames bands[b] .. bands[b + 1] - 1; ``spring`` a scalar or [n_bands]; ``fixed`` [N] or None."""

    def __init__(self, evaluate, positions, offsets, bands, spring=0.1, fixed=None):
        self.evaluate = evaluate
        self.x = np.array(positions, dtype=float).reshape(-1, 3)
        self.off = np.asarray(offsets, dtype=np.int64)
        self.bands = np.asarray(bands, dtype=np.int64)
        nb = len(self.bands) - 1
        self.spring = np.broadcast_to(np.asarray(spring, dtype=float), (nb,)).copy()
        self.fixed = np.zeros(len(self.x), bool) if fixed is None else np.asarray(fixed, bool).copy()
        self.v = np.zeros_like(self.x)
        self.g = np.zeros_like(self.x)              # the NEB force of the last evaluation (0 on end points)
        self.dt = np.zeros(nb)
        self.alpha = np.full(nb, A_START)
        self.n_pos = np.zeros(nb, np.int64)
        self.first = np.ones(nb, bool)
        self.status = np.zeros(nb, np.int64)
        self.steps = np.zeros(nb, np.int64)
        self.crit = np.full(nb, np.nan)
        self.climbing = np.full(nb, -1, np.int64)
        self.e_last = np.full(len(self.off) - 1, np.nan)
        self._forces = None
        self.margins = []            # per evaluation: the smallest margin of the comparisons of the bands that ran
        self.max_dr = 0.0            # the largest |dr| over a band's DOF in any step (tests: <= maxstep)
        self.power = []              # g.v / (|g| |v|) of every power test made: how far from 0 the branch was decided

    def _span(self, b):
        f0, f1 = self.bands[b], self.bands[b + 1]
        return f0, f1 - f0, self.off[f0], self.off[f1]

    def neb_force(self, b, e, F, climb, margins=None):
        """(g [M, n, 3], climbing image or -1, ok) of band b; ok False when a tangent vanishes."""
        f0, M, lo, hi = self._span(b)
        na = (hi - lo) // M
        X = self.x[lo:hi].reshape(M, na, 3)
        Fb = F[lo:hi].reshape(M, na, 3)
        fixed = self.fixed[lo:lo + na]
        E = e[f0:f0 + M]
        ci = -1
        if climb:
            ci = 1 + int(np.argmax(E[1:M - 1]))                         # (the first of equal maxima)
            if margins is not None and M > 3:
                top = np.sort(E[1:M - 1])
                margins.append(top[-1] - top[-2])
        g = np.zeros((M, na, 3))
        ok = True
        for i in range(1, M - 1):
            tp, tm = X[i + 1] - X[i], X[i] - X[i - 1]
            tp[fixed] = 0.0
            tm[fixed] = 0.0
            Fi = np.where(fixed[:, None], 0.0, Fb[i])
            tau = tangent(tp, tm, E[i - 1], E[i], E[i + 1], margins)
            tn = np.sqrt(np.vdot(tau, tau))
            if not (tn > 0.0) or not np.isfinite(tn):
                ok = False
                continue
            that = tau / tn
            ft = np.vdot(Fi, that)
            if i == ci:
                g[i] = Fi - 2.0 * ft * that
            else:
                g[i] = Fi - ft * that + self.spring[b] * (np.sqrt(np.vdot(tp, tp)) - np.sqrt(np.vdot(tm, tm))) * that
        return g, ci, ok

    def _band(self, b, e, F, fmax, climb, dt0, dt_max, maxstep, can_move, margins):
        f0, M, lo, hi = self._span(b)
        na = (hi - lo) // M
        self.e_last[f0:f0 + M] = e[f0:f0 + M]
        finite = np.all(np.isfinite(e[f0:f0 + M])) and np.all(np.isfinite(F[lo:hi]))
        ok = False
        if finite:
            g, ci, ok = self.neb_force(b, e, F, climb, margins)
            ok = ok and np.all(np.isfinite(g))
        if not ok:
            self.status[b], self.crit[b], self.climbing[b] = NONFINITE, np.nan, -1
            return
        self.g[lo:hi] = g.reshape(-1, 3)
        crit = np.sqrt((g * g).sum(-1)).max()
        self.crit[b], self.climbing[b] = crit, ci
        if crit < fmax:
            self.status[b] = CONVERGED
            return
        if not can_move:
            return
        ilo, ihi = lo + na, hi - na                                      # the interior images
        g = g[1:M - 1].reshape(-1, 3)
        v = self.v[ilo:ihi]
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
        self.v[ilo:ihi] = v                                              # (rows of fixed atoms are 0: g is)
        self.x[ilo:ihi] += dr
        self.dt[b] = dt
        self.first[b] = False
        self.steps[b] += 1

    def run(self, max_steps, fmax=0.05, climb=False, dt=0.1, dt_max=1.0, maxstep=0.2):
        """Evaluations 0 .. max_steps; each but the last moves the bands still running.  Returns the energies of every
        evaluation [max_steps + 1 or fewer, n_frames] (the loop stops once no band runs).  A band that converged in an earlier
        run is tested again and moves only if it fails this run's test; a frozen band stays frozen."""
        self.status[self.status == CONVERGED] = RUNNING          # every run tests again: its fmax and climb may differ
        energies = []
        for k in range(max_steps + 1):
            if not (k == 0 and self._forces is not None):
                self._forces = self.evaluate(self.x)
                fresh = True
            else:
                fresh = False
            e, F = self._forces
            margins = []
            for b in range(len(self.bands) - 1):
                if self.status[b] == RUNNING:
                    self._band(b, e, F, fmax, climb, dt, dt_max, maxstep, k < max_steps, margins)
            if fresh or not self.margins:
                self.margins.append(min(margins) if margins else np.inf)
            else:                                                        # the previous run's last evaluation, tested again
                self.margins[-1] = min([self.margins[-1]] + margins)
            energies.append(self.e_last.copy())
            if k < max_steps and np.any(self.status == RUNNING):
                self._forces = None
            if not np.any(self.status == RUNNING):
                break
        return np.array(energies)
