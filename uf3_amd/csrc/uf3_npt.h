// uf3_npt.h -- constant-pressure molecular dynamics on the device (uf3_md_run_npt, include/uf3_hip.h): isotropic
// Martyna-Tobias-Klein dynamics, every frame its own piston.  A frame's cell is s * cell0; v_eps (1/fs) is the rate of ln s.
//
//     dr/dt = v + v_eps r        dv/dt = F/m - (1 + 1/N) v_eps v        ds/dt = v_eps s
//     W_p dv_eps/dt = G = (1 + 1/N) tr K - tr W - 3 P0 V       (K = sum m v (x) v, W = dE/d(strain), both eV)
//
// One step of length dt, h = dt / 2 (tests/_npt_ref.py restates it in NumPy):
//
//     P  v_eps += h G / W_p                                   piston half-kick
//     B  v = a v + b F/m,  a = exp(-x), b = h (1 - exp(-x)) / x,  x = (1 + 1/N) v_eps h      exact kick with the piston's drag
//     A  r = e r + d v,  s = e s,  e = exp(v_eps dt), d = dt (e - 1) / (v_eps dt)            exact drift
//        (with a thermostat: A(h), O on the atoms and on the piston, A(h) with the piston's new rate)
//     -- forces, energy and strain derivative at the new positions and cell --
//     B, P
//
// Between two force calls the closing B P of step t and the opening P B A of step t + 1 are three launches, the shape of
// uf3_relax.h:
//
//   k_npt_partial   one workgroup per chunk of <= 256 atoms of one frame: sum m v^2, sum m v.a, sum m a^2 (a = F/m), eV
//   k_npt_frame     one workgroup per frame: the partials in a fixed order; lane 0 advances v_eps and s (tr K behind the
//                   closing kick follows from the three sums: v' = a v + b F/m), writes the frame's coefficients and its new
//                   cell rows into device memory -- the integrator's own copy and, when the evaluator's persistent lists
//                   are live, the FrameGeom its kernels read -- and the limits of the list test below
//   k_npt_move      one thread per atom: kick, kinetic terms of a thermo step (uf3_md.h's md_store_kin), kick, drift, draws -- k_md_step
//                   with the frame's coefficients in its kick and drift expressions, which stay its own; then the list test: the
//                   reference positions of the evaluator's lists are carried along with the cell (x_ref *= e), and the atom
//                   raises the evaluator's status words when |x - x_ref| has passed the frame's limit
//   k_npt_thermo    one workgroup per frame: uf3_md.h's md_kin_sum, then the record [PE, KE, W (6), K (6), V, s, H]
//
// The list test.  Lists built at r_cut + skin from positions X in a cell C stay complete for positions x in the cell s C
// (s relative to the build) while 2 |x / s - X| <= skin - r_cut (1 / s - 1) for every atom: a pair within r_cut now,
// |x_j + s n C - x_i| <= r_cut, was within r_cut / s + 2 max |x / s - X| at the build.  In today's frame, with x_ref = s X:
// |x - x_ref| <= (s (skin + r_cut) - r_cut) / 2.  The evaluator's own test, |x - x_ref| <= skin / 2, is the stricter one
// when s > 1 and stays in force; this one is the stricter one when s < 1.
//
// Random numbers: the atoms' draws are md_normal3's (counter word 0 = atom index < 2^28); the piston of frame f draws
// from counter word 0 = 2^31 | f, which no atom reaches.  Nothing here uses atomics; a frame's arithmetic depends on the
// frame alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define UF3_NPT_THREADS 256
#define UF3_NPT_REC 17                       // doubles per thermo record

struct NptFrame {                            // one frame's piston (device)
    double s, veps;                         // cell = s cell0; d ln s / dt (1/fs)
    double s_closed, veps_closed;           // ... at the last integer time (what a thermo record reports)
    double s_build;                         // s when the evaluator's lists were last built
    double g_close;                         // G of the last closing half (the opening half of the next run uses the same number)
    double cell0[9], vol0, hgt0[3];         // reference cell, its volume and perpendicular heights
};

struct NptCoef {                             // what k_npt_move needs of its frame's decision
    double a1, b1, a2, b2;                  // closing and opening kick: v = a v + b F/m
    double e1, d1, e2, d2;                  // drift: r = e r + d v (two halves around the O-step with a thermostat)
    double eref;                            // what the cell was scaled by in this launch
    double hard2, soft2;                    // squared limits of the list test; negative: the lists are void (scale out of range)
};

struct NptArgs {
    // per atom
    double *pos, *vel;
    const double *frc, *inv_m;
    double *kin;                            // [7][N] on a thermo step (k_md_step's layout)
    const int *frame_of;
    long long n;
    // chunks
    const int *blk_frame, *blk_n, *frame_blk;
    const long long *blk_lo;
    double *partial;                        // [n_blocks][3]
    // per frame
    const long long *offsets;
    const double *virials;                  // [n_frames][6]
    NptFrame *st;
    NptCoef *coef;
    double *cells;                          // [n_frames][9]: the integrator's copy of the current cells
    FrameGeom *geo;                         // the evaluator's persistent frame geometry (null: no live lists)
    double *pos_ref;                        // ... and the reference positions of its lists (null: no live lists)
    int *flags;                             // the evaluator's status words: [1..4] zeroed here, [2] lists void, [3] early warning
    double dt, p0, tau2_kTp, kT;            // tau2_kTp: tau_p^2 k_B T_p (W_p = (3N + 3) of it)
    double c, cp;                           // exp(-gamma dt) of the atoms and of the piston
    double r_cut, skin;                     // search radius of the lists and their skin
    unsigned long long seed, step;
    int close, open, langevin, thermo;
    int use_g;                              // the opening half takes G from the last closing half (nothing changed since)
    int rebuilt;                            // the lists were built at the state this launch starts from
};

// (1 - exp(-x)) / x and (exp(x) - 1) / x, with their series near 0
__device__ __forceinline__ double npt_phi(double x) {
    return fabs(x) < 1e-4 ? 1.0 - x * (0.5 - x * (1.0 / 6.0 - x * (1.0 / 24.0))) : -expm1(-x) / x;
}
__device__ __forceinline__ double npt_psi(double x) {
    return fabs(x) < 1e-4 ? 1.0 + x * (0.5 + x * (1.0 / 6.0 + x * (1.0 / 24.0))) : expm1(x) / x;
}

__global__ void __launch_bounds__(UF3_NPT_THREADS) k_npt_partial(NptArgs A) {
    __shared__ double lds[3 * UF3_MD_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    double s[3] = {0.0, 0.0, 0.0};
    if (t < A.blk_n[b]) {
        const long long i = A.blk_lo[b] + t;
        const double im = A.inv_m[i], m = UF3_MD_KE / im, ka = im * UF3_MD_ACC;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double v = A.vel[3 * i + k], a = A.frc[3 * i + k] * ka;
            s[0] += m * v * v; s[1] += m * v * a; s[2] += m * a * a;
        }
    }
    md_block_sum<3>(s, lds);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 3; k++) A.partial[3 * b + k] = s[k];
    }
}

__global__ void __launch_bounds__(UF3_NPT_THREADS) k_npt_frame(NptArgs A) {
    __shared__ double lds[3 * UF3_MD_THREADS];
    const int f = blockIdx.x, t = threadIdx.x;
    if (f == 0 && t == 0 && A.open) { A.flags[1] = 0; A.flags[2] = 0; A.flags[3] = 0; A.flags[4] = 0; }
    double q[3] = {0.0, 0.0, 0.0};
    for (int b = A.frame_blk[f] + t; b < A.frame_blk[f + 1]; b += UF3_NPT_THREADS) {
#pragma unroll
        for (int k = 0; k < 3; k++) q[k] += A.partial[3 * b + k];
    }
    md_block_sum<3>(q, lds);
    if (t != 0) return;
    NptFrame *S = A.st + f;
    NptCoef *K = A.coef + f;
    const double n = (double)(A.offsets[f + 1] - A.offsets[f]);
    const double alpha = 1.0 + 1.0 / n, wp = (3.0 * n + 3.0) * A.tau2_kTp, h = 0.5 * A.dt;
    const double trw = A.virials[6 * f] + A.virials[6 * f + 1] + A.virials[6 * f + 2];
    double s = S->s, ve = S->veps, g;
    if (A.rebuilt) S->s_build = s;
    K->a1 = 1.0; K->b1 = 0.0; K->a2 = 1.0; K->b2 = 0.0;
    K->e1 = 1.0; K->d1 = 0.0; K->e2 = 1.0; K->d2 = 0.0; K->eref = 1.0; K->hard2 = 0.0; K->soft2 = 0.0;
    if (A.close) {
        const double x = alpha * ve * h, a1 = exp(-x), b1 = h * npt_phi(x);
        const double trk = a1 * a1 * q[0] + 2.0 * a1 * b1 * q[1] + b1 * b1 * q[2];
        g = alpha * trk - trw - 3.0 * A.p0 * (S->vol0 * s * s * s);
        ve += h * g / wp;
        K->a1 = a1; K->b1 = b1;
        S->g_close = g;
        S->s_closed = s; S->veps_closed = ve;
    } else {
        g = A.use_g ? S->g_close : alpha * q[0] - trw - 3.0 * A.p0 * (S->vol0 * s * s * s);
        S->s_closed = s; S->veps_closed = ve;
    }
    if (A.open) {
        ve += h * g / wp;
        const double x = alpha * ve * h;
        K->a2 = exp(-x); K->b2 = h * npt_phi(x);
        double eref;
        if (A.langevin) {
            const double y1 = ve * h, e1 = exp(y1);
            K->e1 = e1; K->d1 = h * npt_psi(y1);
            const double2 xi = md_normal2(A.seed, (long long)(0x80000000u | (unsigned)f), A.step, 0);
            ve = A.cp * ve + sqrt((1.0 - A.cp * A.cp) * A.kT / wp) * xi.x;
            const double y2 = ve * h, e2 = exp(y2);
            K->e2 = e2; K->d2 = h * npt_psi(y2);
            s = s * e1; s = s * e2;
            eref = e1 * e2;
        } else {
            const double y = ve * A.dt, e1 = exp(y);
            K->e1 = e1; K->d1 = A.dt * npt_psi(y);
            s = s * e1;
            eref = e1;
        }
        K->eref = eref;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const double ck = s * S->cell0[k];
            A.cells[9 * f + k] = ck;
            if (A.geo) A.geo[f].cell[k] = ck;
        }
        // the list test's limits at the new scale (relative to the build), and the range of scales over which the image range
        // of the build's frame geometry (fac = ceil(r_cut / height) per axis) is the one a build at the new cell would find
        const double sr = s / S->s_build;
        double lim = 0.5 * (sr * (A.skin + A.r_cut) - A.r_cut) * (1.0 - 1e-9);
        bool ok = lim > 0.0 && isfinite(s) && s > 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double fb = ceil(A.r_cut / (S->s_build * S->hgt0[k])), now = A.r_cut / (s * S->hgt0[k]);
            ok = ok && now > fb - 1.0 + 1e-9 && now < fb - 1e-9;
        }
        K->hard2 = ok ? lim * lim : -1.0;
        K->soft2 = ok ? 0.49 * lim * lim : -1.0;
    }
    S->s = s; S->veps = ve;
}

template <bool LANGEVIN, bool THERMO>
__global__ void __launch_bounds__(UF3_NPT_THREADS) k_npt_move(NptArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const NptCoef *K = A.coef + A.frame_of[i];
    const double im = A.inv_m[i], ka = im * UF3_MD_ACC;
    double v[3], a[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { v[k] = A.vel[3 * i + k]; a[k] = A.frc[3 * i + k] * ka; }
    if (A.close) {
        const double a1 = K->a1, b1 = K->b1;
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] = a1 * v[k] + b1 * a[k];
    }
    if (THERMO) md_store_kin(A.kin, A.n, i, im, v);
    if (A.open) {
        const double a2 = K->a2, b2 = K->b2, e1 = K->e1, d1 = K->d1;
        double x[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { x[k] = A.pos[3 * i + k]; v[k] = a2 * v[k] + b2 * a[k]; }
        if (LANGEVIN) {
            double xi[3];
            md_normal3(A.seed, i, A.step, 0, xi);
            const double sig = sqrt((1.0 - A.c * A.c) * A.kT * ka), e2 = K->e2, d2 = K->d2;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                x[k] = e1 * x[k] + d1 * v[k];
                v[k] = A.c * v[k] + sig * xi[k];
                x[k] = e2 * x[k] + d2 * v[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) x[k] = e1 * x[k] + d1 * v[k];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) A.pos[3 * i + k] = x[k];
        if (A.pos_ref) {
            const double eref = K->eref;
            double moved = 0.0;
#pragma unroll
            for (int k = 0; k < 3; k++) {
                const double xr = A.pos_ref[3 * i + k] * eref;
                A.pos_ref[3 * i + k] = xr;
                moved += (x[k] - xr) * (x[k] - xr);
            }
            if (!(moved <= K->hard2)) A.flags[2] = 1;
            if (!(moved <= K->soft2)) A.flags[3] = 1;
        }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) A.vel[3 * i + k] = v[k];
}

// one record per frame: [PE, KE, W (6), K (6), V, s, H = KE + PE + P0 V + W_p v_eps^2 / 2] at the integer time just closed
__global__ void __launch_bounds__(UF3_MD_THREADS) k_npt_thermo(NptArgs A, const double *energies, double *rec_base) {
    const int f = blockIdx.x;
    const long long lo = A.offsets[f], hi = A.offsets[f + 1];
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    md_kin_sum(A.kin, A.n, lo, hi, UF3_NPT_REC, s);
    if (threadIdx.x == 0) {
        const NptFrame *S = A.st + f;
        double *r = rec_base + (size_t)f * UF3_NPT_REC;
        const double n = (double)(hi - lo), wp = (3.0 * n + 3.0) * A.tau2_kTp;
        const double sc = S->s_closed, vol = S->vol0 * sc * sc * sc;
        r[0] = energies[f];
        r[1] = s[0];
        for (int k = 0; k < 6; k++) { r[2 + k] = A.virials[6 * f + k]; r[8 + k] = s[1 + k]; }
        r[14] = vol;
        r[15] = sc;
        r[16] = s[0] + energies[f] + A.p0 * vol + 0.5 * wp * S->veps_closed * S->veps_closed;
    }
}
