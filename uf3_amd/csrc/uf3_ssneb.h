// uf3_ssneb.h -- nudged elastic bands whose images differ in cell (uf3_ssneb_create, include/uf3_hip.h): uf3_neb.h's band in
// uf3_relax.h's generalised coordinates.  The band's reference cell C0 is the cell of its image 0; image i has D_i = C0^-1 C_i,
// q_i = x_i D_i^-1 and the vector u_i = (q_i [n][3], Y_i = kappa D_i [3][3]) of 3 n + 9 numbers, kappa the band's cell factor.
// The generalised true force is (F D^T, G = -D^-T W / kappa), W the strain derivative of uf3_eval_virial.  Tangents, springs, the
// climbing image and the one FIRE per band are uf3_neb.h's rules on these longer vectors (differences as stored); the band's
// state machine is k_neb_band itself, which sees the cell only through the image sums and the chunk maxima.  A step's launches:
//
//   k_ssneb_partial  one 256-thread workgroup per chunk of <= 256 atoms of one image: F D^T per atom (kept: uf3_neb_get_state's
//                    forces), the chunk's ten dot products among {t+, t-, F D^T, v} over its atoms (t+- from q) and the NaN flag.
//                    The image's first chunk also leaves G and the image's D and cell velocity as they are at this evaluation.
//   k_ssneb_force    one workgroup per chunk: the image's sums from its chunks' partials in a fixed order, then the nine cell
//                    entries of t+, t-, G and vc once per image, entry by entry; from there k_neb_force's rules.  g per atom, the
//                    chunk's largest |g_i|^2 (the image's first chunk: also over the three rows of the cell part), and from one
//                    writer per image the cell part of g and the image's sums.
//   k_neb_band       (uf3_neb.h, unchanged)
//   k_ssneb_move     one thread per atom: mix, kick, scale; q += dr, x = q D_new with D_new = D + dr_Y / kappa formed by every
//                    thread from the evaluation's D, vc and cell g (read only here); the thread of an image's first atom writes
//                    D, vc and the cell C0 D_new.  End images are never written.
//
// No atomics; a band's arithmetic depends on that band alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uf3_neb.h"

struct SsChunkArgs {                        // k_ssneb_partial and k_ssneb_force
    const double *q, *frc, *vel;           // [N][3]: scaled coordinates, the evaluator's forces, the velocities of q
    const double *virials;                 // [n_frames][6]
    const double *D, *vc;                  // [n_frames][9]: the deformations and the velocities of Y
    const double *kappa;                   // [n_bands]
    const int *blk_frame;                  // the chunk table and the bands, as NebChunkArgs
    const long long *blk_lo;
    const int *blk_n;
    const int *frame_blk;
    const int *frame_band;
    const long long *offsets;
    const double *energies;
    const NebBand *bands;
    double *fq;                            // [N][3]: F D^T
    double *G, *D_ev, *vc_ev;              // [n_frames][9]: the cell force, and D and vc at this evaluation (k_ssneb_move's input)
    double *partial;                       // [n_blocks][UF3_NEB_NSUM]
    double *g;                             // [N][3]: the atom rows of the NEB force
    double *gc;                            // [n_frames][9]: its cell part (0 on end points and images without a tangent)
    double *cmax;                          // [n_blocks]
    NebImage *img;                         // [n_frames]
    int climb;
    int all;
};

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_ssneb_partial(SsChunkArgs A) {
    __shared__ double lds[UF3_NEB_NSUM * UF3_RELAX_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int f = A.blk_frame[b];
    const int bd = A.frame_band[f];
    const NebBand *B = A.bands + bd;
    if (!A.all && B->status != UF3_RELAX_RUNNING) return;
    const bool interior = f > B->frame0 && f < B->frame0 + B->n_img - 1;
    double D[9];
#pragma unroll
    for (int k = 0; k < 9; k++) D[k] = A.D[9 * f + k];
    if (b == A.frame_blk[f] && t == 0) {                // one writer per image: G = -D^-T W / kappa (not finite for a singular D)
        const double *v = A.virials + 6 * f;
        const double W[9] = {v[0], v[5], v[4], v[5], v[1], v[3], v[4], v[3], v[2]};
        const double kap = A.kappa[bd];
        double Di[9];
        relax_inv3(D, Di);
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                A.G[9 * f + 3 * i + j] = -(Di[i] * W[j] + Di[3 + i] * W[3 + j] + Di[6 + i] * W[6 + j]) / kap;
        for (int k = 0; k < 9; k++) { A.D_ev[9 * f + k] = D[k]; A.vc_ev[9 * f + k] = A.vc[9 * f + k]; }
    }
    double s[UF3_NEB_NSUM];
#pragma unroll
    for (int k = 0; k < UF3_NEB_NSUM; k++) s[k] = 0.0;
    if (t < A.blk_n[b]) {
        const long long i = A.blk_lo[b] + t;
        double Fx[3], F[3];
#pragma unroll
        for (int k = 0; k < 3; k++) Fx[k] = A.frc[3 * i + k];
        relax_g(Fx, D, true, false, F);
#pragma unroll
        for (int k = 0; k < 3; k++) A.fq[3 * i + k] = F[k];
        const double fx2 = Fx[0] * Fx[0] + Fx[1] * Fx[1] + Fx[2] * Fx[2];
        const double f2 = F[0] * F[0] + F[1] * F[1] + F[2] * F[2];
        s[10] = (isfinite(fx2) && isfinite(f2)) ? 0.0 : __builtin_nan("");
        if (interior) {
            double p[3], m[3], v[3];
            neb_diffs(A.q, i, A.offsets[f + 1] - A.offsets[f], p, m);
#pragma unroll
            for (int k = 0; k < 3; k++) v[k] = A.vel[3 * i + k];
            s[0] = p[0] * p[0] + p[1] * p[1] + p[2] * p[2];
            s[1] = p[0] * m[0] + p[1] * m[1] + p[2] * m[2];
            s[2] = m[0] * m[0] + m[1] * m[1] + m[2] * m[2];
            s[3] = F[0] * p[0] + F[1] * p[1] + F[2] * p[2];
            s[4] = F[0] * m[0] + F[1] * m[1] + F[2] * m[2];
            s[5] = f2;
            s[6] = v[0] * p[0] + v[1] * p[1] + v[2] * p[2];
            s[7] = v[0] * m[0] + v[1] * m[1] + v[2] * m[2];
            s[8] = v[0] * F[0] + v[1] * F[1] + v[2] * F[2];
            s[9] = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        }
    }
    relax_block_reduce<UF3_NEB_NSUM>(s, lds);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < UF3_NEB_NSUM; k++) A.partial[UF3_NEB_NSUM * b + k] = s[k];
    }
}

// entry k of the cell parts of t+ and t- of interior image f: Y = kappa D, as stored
__device__ __forceinline__ void ssneb_cell_diffs(const double *D, int f, int k, double kap, double &p, double &m) {
    const double y = kap * D[9 * f + k];
    p = kap * D[9 * (f + 1) + k] - y;
    m = y - kap * D[9 * (f - 1) + k];
}

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_ssneb_force(SsChunkArgs A) {
    __shared__ double lds[UF3_NEB_NSUM * UF3_RELAX_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int f = A.blk_frame[b];
    const int bd = A.frame_band[f];
    const NebBand *B = A.bands + bd;
    if (!A.all && B->status != UF3_RELAX_RUNNING) return;
    const bool interior = f > B->frame0 && f < B->frame0 + B->n_img - 1;
    const bool first = b == A.frame_blk[f];             // the image's first chunk carries its cell rows
    const bool lead = first && t == 0;                  // one writer per image
    double s[UF3_NEB_NSUM];
#pragma unroll
    for (int k = 0; k < UF3_NEB_NSUM; k++) s[k] = 0.0;
    for (int c = A.frame_blk[f] + t; c < A.frame_blk[f + 1]; c += UF3_RELAX_THREADS) {
#pragma unroll
        for (int k = 0; k < UF3_NEB_NSUM - 1; k++) s[k] += A.partial[UF3_NEB_NSUM * c + k];
        s[10] = relax_nanmax(s[10], A.partial[UF3_NEB_NSUM * c + 10]);
    }
    relax_block_reduce<UF3_NEB_NSUM>(s, lds);
    const double kap = A.kappa[bd];
    const double *G = A.G + 9 * f;
    bool gfin = true;
    for (int k = 0; k < 9; k++) gfin = gfin && isfinite(G[k]);
    int bad = (s[10] != s[10] || !gfin) ? UF3_NEB_BAD_FORCE : 0;
    const long long i = A.blk_lo[b] + t;
    const bool mine = t < A.blk_n[b];
    if (!interior) {
        if (lead) {
            NebImage I = {0.0, 0.0, 0.0, 0.0, 0.0, bad, 0};
            A.img[f] = I;
            for (int k = 0; k < 9; k++) A.gc[9 * f + k] = 0.0;
        }
        if (mine) {
#pragma unroll
            for (int k = 0; k < 3; k++) A.g[3 * i + k] = 0.0;
        }
        return;
    }
    // the nine cell entries, once per image, after the chunk sums, entry by entry (every thread: the same bits)
    for (int k = 0; k < 9; k++) {
        double p, m;
        ssneb_cell_diffs(A.D, f, k, kap, p, m);
        const double Gk = G[k], vk = A.vc[9 * f + k];
        s[0] += p * p; s[1] += p * m; s[2] += m * m;
        s[3] += Gk * p; s[4] += Gk * m; s[5] += Gk * Gk;
        s[6] += vk * p; s[7] += vk * m; s[8] += vk * Gk; s[9] += vk * vk;
    }
    const double Em = A.energies[f - 1], E0 = A.energies[f], Ep = A.energies[f + 1];
    double wp, wm;
    if (Ep > E0 && E0 > Em) { wp = 1.0; wm = 0.0; }
    else if (Ep < E0 && E0 < Em) { wp = 0.0; wm = 1.0; }
    else {
        const double dp = fabs(Ep - E0), dm = fabs(Em - E0);
        const double dmax = dp > dm ? dp : dm, dmin = dp > dm ? dm : dp;
        if (Ep > Em) { wp = dmax; wm = dmin; } else { wp = dmin; wm = dmax; }
    }
    const double pp = s[0], pm = s[1], mm = s[2], Fp = s[3], Fm = s[4], FF = s[5], vp = s[6], vm = s[7], vF = s[8], vv = s[9];
    const double tau2 = wp * wp * pp + 2.0 * wp * wm * pm + wm * wm * mm;
    if (!(tau2 > 0.0) || !isfinite(tau2)) bad |= UF3_NEB_BAD_TANGENT;
    const double itau = 1.0 / sqrt(tau2);
    const double Ft = (wp * Fp + wm * Fm) * itau;
    const bool climbs = neb_climbing(A.energies, B, A.climb) == f - B->frame0;
    const double c = climbs ? -2.0 * Ft : B->spring * (sqrt(pp) - sqrt(mm)) - Ft;
    const double cp = c * wp * itau, cm = c * wm * itau;
    const bool tangent = !(bad & UF3_NEB_BAD_TANGENT);
    if (lead) {
        NebImage I;
        I.cp = cp; I.cm = cm;
        I.gv = vF + cp * vp + cm * vm;
        I.gg = FF + cp * cp * pp + cm * cm * mm + 2.0 * (cp * Fp + cm * Fm + cp * cm * pm);
        I.vv = vv;
        I.bad = bad; I.pad = 0;
        A.img[f] = I;
    }
    double m2[1] = {0.0};
    if (mine) {
        double g[3] = {0.0, 0.0, 0.0};
        if (tangent) {
            double p[3], m[3];
            neb_diffs(A.q, i, A.offsets[f + 1] - A.offsets[f], p, m);
#pragma unroll
            for (int k = 0; k < 3; k++) g[k] = A.fq[3 * i + k] + cp * p[k] + cm * m[k];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) A.g[3 * i + k] = g[k];
        m2[0] = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    }
    if (first && t < 3) {                               // row t of the cell part of g
        double r2 = 0.0;
        for (int k = 3 * t; k < 3 * t + 3; k++) {
            double p, m, gk = 0.0;
            ssneb_cell_diffs(A.D, f, k, kap, p, m);
            if (tangent) gk = G[k] + cp * p + cm * m;
            A.gc[9 * f + k] = gk;
            r2 += gk * gk;
        }
        m2[0] = relax_nanmax(m2[0], r2);
    }
    relax_block_reduce<1>(m2, lds);
    if (t == 0) A.cmax[b] = m2[0];
}

struct SsMoveArgs {
    double *pos, *q, *vel;                 // [N][3]
    double *D, *vc, *cells;                // [n_frames][9]
    const double *g;                       // [N][3]
    const double *gc, *D_ev, *vc_ev;       // [n_frames][9]
    const double *kappa;                   // [n_bands]
    const int *frame_of;                   // [N]
    const int *frame_band;                 // [n_frames]
    const long long *offsets;              // [n_frames + 1]
    const NebBand *bands;
    const NebCoef *coef;
    long long n;
};

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_ssneb_move(SsMoveArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const int f = A.frame_of[i], bd = A.frame_band[f];
    const NebCoef *K = A.coef + bd;
    const NebBand *B = A.bands + bd;
    if (!K->move || f == B->frame0 || f == B->frame0 + B->n_img - 1) return;
    const double a = K->a, b = K->b, dt = K->dt, s = K->s, kap = A.kappa[bd];
    const bool scale = K->scale != 0;
    double Dn[9], vn[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        const double g = A.gc[9 * f + k];
        const double v = (a * A.vc_ev[9 * f + k] + b * g) + dt * g;
        vn[k] = v;
        double dr = dt * v;
        if (scale) dr *= s;
        Dn[k] = A.D_ev[9 * f + k] + dr / kap;
    }
    double q[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double g = A.g[3 * i + k];
        const double v = (a * A.vel[3 * i + k] + b * g) + dt * g;
        A.vel[3 * i + k] = v;
        double dr = dt * v;
        if (scale) dr *= s;
        q[k] = A.q[3 * i + k] + dr;
        A.q[3 * i + k] = q[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) A.pos[3 * i + k] = q[0] * Dn[k] + q[1] * Dn[3 + k] + q[2] * Dn[6 + k];
    if (i == A.offsets[f]) {                            // one writer per image; C0 is the cell of the band's first image
        const double *C0 = A.cells + 9 * (size_t)B->frame0;
#pragma unroll
        for (int k = 0; k < 9; k++) { A.D[9 * f + k] = Dn[k]; A.vc[9 * f + k] = vn[k]; }
        for (int r = 0; r < 3; r++)
            for (int j = 0; j < 3; j++)
                A.cells[9 * f + 3 * r + j] = C0[3 * r] * Dn[j] + C0[3 * r + 1] * Dn[3 + j] + C0[3 * r + 2] * Dn[6 + j];
    }
}
