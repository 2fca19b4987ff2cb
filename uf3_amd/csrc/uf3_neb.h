// uf3_neb.h -- batched nudged elastic bands on the device (uf3_neb_*, include/uf3_hip.h): a band is M >= 3 consecutive frames of
// the batch (images; the first and the last are end points and never move), the improved tangent of Henkelman & Jonsson (2000),
// optionally a climbing image, and one FIRE (uf3_relax.h's constants and rules) over the band's whole interior vector.  The
// forces come from the evaluator (eval_impl) before the four launches of a step (k_neb_rearm, once per run, makes converged bands
// run again: they are tested against this run's fmax and climb at its first evaluation and move only if they fail it):
//
//   k_neb_partial  one 256-thread workgroup per chunk of <= 256 atoms of one image (chunks never straddle frames): the chunk's ten
//                  dot products among {t+, t-, F, v} (t+ = R_{i+1} - R_i, t- = R_i - R_{i-1}, as stored) and a NaN flag for a
//                  force that is not finite.  |tau|^2, F.tau, g.v, |g|^2 and |v|^2 follow from them for any tangent weights.
//   k_neb_force    one workgroup per chunk: the image's sums from its chunks' partials in a fixed order (every chunk of an image
//                  repeats them and gets the same bits), the tangent weights from the energies, the climbing image, the
//                  coefficients of g = F + c+ t+ + c- t-; then g per atom (kept: uf3_neb_get_state's neb_forces, the move's
//                  input) and the chunk's largest |g_i|^2.  The image's first chunk leaves c+, c-, g.v, |g|^2, |v|^2.
//   k_neb_band     one workgroup per band: the criterion from the chunks' maxima, the band's sums image by image, the convergence
//                  test and FIRE's state machine on lane 0, the move's coefficients
//   k_neb_move     one thread per atom: mix, kick, scale, move (interior images of a band that moves)
//
// Nothing here uses atomics: chunk partials, then a strided pass, then an LDS tree, and image by image in a loop.  A band's
// arithmetic depends on that band alone (chunks start at an image's first atom), never on the batch around it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uf3_relax.h"

#define UF3_NEB_NSUM 11                     // pp, pm, mm, Fp, Fm, FF, vp, vm, vF, vv and the NaN flag
#define UF3_NEB_BAD_FORCE 1                 // NebImage::bad
#define UF3_NEB_BAD_TANGENT 2

struct NebBand {                            // one band's optimiser state (device)
    double dt, alpha, spring, crit_last;   // crit_last: the criterion at the last evaluation while running
    long long steps;
    int n_pos, first, status, climbing;    // climbing: the image (index within the band) that climbed at that evaluation, or -1
    int frame0, n_img;                     // the band's first frame and its number of images
};

struct NebImage {                           // what k_neb_force leaves of one image for k_neb_band
    double cp, cm, gv, gg, vv;             // g = F + cp t+ + cm t-; g.v, |g|^2, |v|^2 over the image
    int bad, pad;
};

struct NebCoef {                            // what k_neb_move needs of its band's decision in this step
    double a, b, dt, s;                    // v' = (a v + b g) + dt g; dr = dt v' (* s when the trust radius cuts)
    int move, scale;
};

struct NebChunkArgs {                       // k_neb_partial and k_neb_force
    const double *pos, *frc, *vel;         // [N][3]
    const uint8_t *fixed;                  // [N] or null
    const int *blk_frame;                  // [n_blocks]
    const long long *blk_lo;               // [n_blocks]: the chunk's first atom
    const int *blk_n;                      // [n_blocks]: atoms in the chunk (<= 256)
    const int *frame_blk;                  // [n_frames + 1]: the frame's chunks
    const int *frame_band;                 // [n_frames]
    const long long *offsets;              // [n_frames + 1]
    const double *energies;                // [n_frames]
    const NebBand *bands;
    double *partial;                       // [n_blocks][UF3_NEB_NSUM]
    double *g;                             // [N][3]: the NEB force (0 on end points, fixed atoms, images without a tangent)
    double *cmax;                          // [n_blocks]: the chunk's largest |g_i|^2
    NebImage *img;                         // [n_frames]
    int climb;
    int all;                               // also the bands that do not run (uf3_neb_get_state's neb_forces)
};

// t+ and t- of atom i of an interior image whose frame holds na atoms (the images of a band are consecutive frames)
__device__ __forceinline__ void neb_diffs(const double *pos, long long i, long long na, double p[3], double m[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double x = pos[3 * i + k];
        p[k] = pos[3 * (i + na) + k] - x;
        m[k] = x - pos[3 * (i - na) + k];
    }
}

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_neb_partial(NebChunkArgs A) {
    __shared__ double lds[UF3_NEB_NSUM * UF3_RELAX_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int f = A.blk_frame[b];
    const NebBand *B = A.bands + A.frame_band[f];
    if (!A.all && B->status != UF3_RELAX_RUNNING) return;
    const bool interior = f > B->frame0 && f < B->frame0 + B->n_img - 1;
    double s[UF3_NEB_NSUM];
#pragma unroll
    for (int k = 0; k < UF3_NEB_NSUM; k++) s[k] = 0.0;
    if (t < A.blk_n[b]) {
        const long long i = A.blk_lo[b] + t;
        double F[3];
#pragma unroll
        for (int k = 0; k < 3; k++) F[k] = A.frc[3 * i + k];
        const double f2 = F[0] * F[0] + F[1] * F[1] + F[2] * F[2];
        s[10] = isfinite(f2) ? 0.0 : __builtin_nan("");
        if (interior && !(A.fixed && A.fixed[i])) {
            double p[3], m[3], v[3];
            neb_diffs(A.pos, i, A.offsets[f + 1] - A.offsets[f], p, m);
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

// the interior image of highest energy, ties to the lowest index (image index within the band; -1 without climbing)
__device__ __forceinline__ int neb_climbing(const double *energies, const NebBand *B, int climb) {
    if (!climb) return -1;
    int best = 1;
    double eb = energies[B->frame0 + 1];
    for (int j = 2; j < B->n_img - 1; j++) {
        const double e = energies[B->frame0 + j];
        if (e > eb) { eb = e; best = j; }
    }
    return best;
}

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_neb_force(NebChunkArgs A) {
    __shared__ double lds[UF3_NEB_NSUM * UF3_RELAX_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int f = A.blk_frame[b];
    const NebBand *B = A.bands + A.frame_band[f];
    if (!A.all && B->status != UF3_RELAX_RUNNING) return;
    const bool interior = f > B->frame0 && f < B->frame0 + B->n_img - 1;
    const bool lead = b == A.frame_blk[f] && t == 0;    // one writer per image
    // the image's sums: its chunks in a strided pass, then the tree (the same bits in every chunk of the image)
    double s[UF3_NEB_NSUM];
#pragma unroll
    for (int k = 0; k < UF3_NEB_NSUM; k++) s[k] = 0.0;
    for (int c = A.frame_blk[f] + t; c < A.frame_blk[f + 1]; c += UF3_RELAX_THREADS) {
#pragma unroll
        for (int k = 0; k < UF3_NEB_NSUM - 1; k++) s[k] += A.partial[UF3_NEB_NSUM * c + k];
        s[10] = relax_nanmax(s[10], A.partial[UF3_NEB_NSUM * c + 10]);
    }
    relax_block_reduce<UF3_NEB_NSUM>(s, lds);
    int bad = (s[10] != s[10]) ? UF3_NEB_BAD_FORCE : 0;
    const long long i = A.blk_lo[b] + t;
    const bool mine = t < A.blk_n[b];
    if (!interior) {
        if (lead) { NebImage I = {0.0, 0.0, 0.0, 0.0, 0.0, bad, 0}; A.img[f] = I; }
        if (mine) {
#pragma unroll
            for (int k = 0; k < 3; k++) A.g[3 * i + k] = 0.0;
        }
        return;
    }
    // the tangent's weights: tau = wp t+ + wm t-
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
    const double Ft = (wp * Fp + wm * Fm) * itau;                       // F . tau^
    const bool climbs = neb_climbing(A.energies, B, A.climb) == f - B->frame0;
    const double c = climbs ? -2.0 * Ft : B->spring * (sqrt(pp) - sqrt(mm)) - Ft;
    const double cp = c * wp * itau, cm = c * wm * itau;
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
        if (!(bad & UF3_NEB_BAD_TANGENT) && !(A.fixed && A.fixed[i])) {      // (no tangent, no NEB force: g = 0, the band freezes)
            double p[3], m[3];
            neb_diffs(A.pos, i, A.offsets[f + 1] - A.offsets[f], p, m);
#pragma unroll
            for (int k = 0; k < 3; k++) g[k] = A.frc[3 * i + k] + cp * p[k] + cm * m[k];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) A.g[3 * i + k] = g[k];
        m2[0] = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    }
    relax_block_reduce<1>(m2, lds);
    if (t == 0) A.cmax[b] = m2[0];
}

struct NebBandArgs {
    const double *cmax;                    // [n_blocks]
    const int *frame_blk;                  // [n_frames + 1]
    const double *energies;                // [n_frames]
    const NebImage *img;                   // [n_frames]
    NebBand *bands;
    NebCoef *coef;                         // [n_bands]
    double *e_last;                        // [n_frames]: the energies at the band's last evaluation while running
    double *rec;                           // this step's record row [n_frames + 2 n_bands] or null
    double fmax, dt0, dt_max, maxstep;     // dt0: the time step of a band's first move (later moves carry their own)
    int n_frames;
    int climb;
    int can_move;                          // 0 on the run's last evaluation: the convergence test only
};

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_neb_band(NebBandArgs A) {
    __shared__ double lds[UF3_RELAX_THREADS];
    const int bd = blockIdx.x, t = threadIdx.x;
    NebBand *B = A.bands + bd;
    NebCoef *K = A.coef + bd;
    const int f0 = B->frame0, M = B->n_img;
    if (B->status == UF3_RELAX_RUNNING) {
        double m2[1] = {0.0};
        for (int c = A.frame_blk[f0 + 1] + t; c < A.frame_blk[f0 + M - 1]; c += UF3_RELAX_THREADS)
            m2[0] = relax_nanmax(m2[0], A.cmax[c]);
        relax_block_reduce<1>(m2, lds);
        for (int j = t; j < M; j += UF3_RELAX_THREADS) A.e_last[f0 + j] = A.energies[f0 + j];
        if (t == 0) {
            double GV = 0.0, GG = 0.0, VV = 0.0;
            bool finite = true;
            for (int j = 0; j < M; j++) {                               // image by image: the band's order
                const NebImage *I = A.img + f0 + j;
                finite = finite && isfinite(A.energies[f0 + j]) && I->bad == 0;
                if (j > 0 && j < M - 1) { GV += I->gv; GG += I->gg; VV += I->vv; }
            }
            const double crit = sqrt(m2[0]);
            finite = finite && isfinite(GV) && isfinite(GG) && isfinite(VV) && isfinite(crit);
            B->crit_last = finite ? crit : __builtin_nan("");
            B->climbing = finite ? neb_climbing(A.energies, B, A.climb) : -1;
            int move = 0;
            if (!finite) {
                B->status = UF3_RELAX_NONFINITE;
            } else if (crit < A.fmax) {
                B->status = UF3_RELAX_CONVERGED;
            } else if (A.can_move) {
                double a = 1.0, b = 0.0, dt = B->first ? A.dt0 : B->dt, alpha = B->alpha;
                int n_pos = B->n_pos;
                if (!B->first) {
                    if (GV > 0.0) {
                        a = 1.0 - alpha;
                        b = alpha * sqrt(VV) / sqrt(GG);
                        if (n_pos > UF3_FIRE_NMIN) { dt = fmin(dt * UF3_FIRE_FINC, A.dt_max); alpha *= UF3_FIRE_FA; }
                        n_pos += 1;
                    } else {
                        a = 0.0; b = 0.0;
                        alpha = UF3_FIRE_ASTART; dt *= UF3_FIRE_FDEC; n_pos = 0;
                    }
                }
                // |v'|^2 of v' = a v + (b + dt) g from the band's sums
                const double c = b + dt;
                const double v2 = fmax(a * a * VV + 2.0 * a * c * GV + c * c * GG, 0.0);
                const double drn = dt * sqrt(v2);
                const int scale = drn > A.maxstep;
                B->dt = dt; B->alpha = alpha; B->n_pos = n_pos; B->first = 0; B->steps += 1;
                K->a = a; K->b = b; K->dt = dt; K->s = scale ? A.maxstep / drn : 1.0; K->scale = scale;
                move = 1;
            }
            K->move = move;
        }
    } else if (t == 0) {
        K->move = 0;
    }
    if (A.rec) {
        __syncthreads();
        for (int j = t; j < M; j += UF3_RELAX_THREADS) A.rec[f0 + j] = A.e_last[f0 + j];
        if (t == 0) {
            A.rec[A.n_frames + 2 * bd] = B->crit_last;
            A.rec[A.n_frames + 2 * bd + 1] = (double)B->climbing;
        }
    }
}

// a run's first launch: convergence is a statement about one run's fmax and climb, so every run tests again
__global__ void k_neb_rearm(NebBand *bands, int n_bands) {
    const int bd = blockIdx.x * blockDim.x + threadIdx.x;
    if (bd < n_bands && bands[bd].status == UF3_RELAX_CONVERGED) bands[bd].status = UF3_RELAX_RUNNING;
}

struct NebMoveArgs {
    double *pos, *vel;                     // [N][3]
    const double *g;
    const uint8_t *fixed;
    const int *frame_of;                   // [N]
    const int *frame_band;                 // [n_frames]
    const NebBand *bands;
    const NebCoef *coef;
    long long n;
};

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_neb_move(NebMoveArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const int f = A.frame_of[i], bd = A.frame_band[f];
    const NebCoef *K = A.coef + bd;
    const NebBand *B = A.bands + bd;
    if (!K->move || f == B->frame0 || f == B->frame0 + B->n_img - 1 || (A.fixed && A.fixed[i])) return;
    const double a = K->a, b = K->b, dt = K->dt, s = K->s;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double g = A.g[3 * i + k];
        const double v = (a * A.vel[3 * i + k] + b * g) + dt * g;
        A.vel[3 * i + k] = v;
        double dr = dt * v;
        if (K->scale) dr *= s;
        A.pos[3 * i + k] += dr;
    }
}
