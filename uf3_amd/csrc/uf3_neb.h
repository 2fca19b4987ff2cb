// uf3_neb.h -- batched nudged elastic bands on the device (uf3_neb_*, include/uf3_hip.h): a band is M >= 3 consecutive frames of
// the batch (images; the first and the last are end points and never move), the improved tangent of Henkelman & Jonsson (2000),
// optionally a climbing image, and one FIRE (uf3_relax.h's fire_step and fire_kick) over the band's whole interior vector.  The
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
//
// Bands whose images differ in cell (uf3_ssneb_create) are the <true> instances of the same three kernels: the band in
// uf3_relax.h's generalised coordinates.  The band's reference cell C0 is the cell of its image 0; image i has D_i = C0^-1 C_i,
// q_i = x_i D_i^-1 and the vector u_i = (q_i [n][3], Y_i = kappa D_i [3][3]) of 3 n + 9 numbers, kappa the band's cell factor.
// The generalised true force is (F D^T, G = relax_cell_force).  Tangents, springs, the climbing image and the one FIRE per band
// are the same rules on these longer vectors (differences as stored); k_neb_band sees the cell only through the image sums and
// the chunk maxima.  What the cell instances add:
//
//   k_neb_partial  F D^T per atom (kept: uf3_neb_get_state's forces) in the place of F, t+- from q.  The image's first chunk also
//                  leaves G and the image's D and cell velocity as they are at this evaluation.
//   k_neb_force    after the chunk sums, the nine cell entries of t+, t-, G and vc once per image, entry by entry.  The image's
//                  first chunk: the cell part of g, and its three rows in the chunk's largest |g_i|^2.
//   k_neb_move     q += dr, x = q D_new with D_new = D + dr_Y / kappa formed by every thread from the evaluation's D, vc and cell
//                  g (read only here); the thread of an image's first atom writes D, vc and the cell C0 D_new.  End images are
//                  never written.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "uf3_relax.h"

#define UF3_NEB_NSUM 11                     // pp, pm, mm, Fp, Fm, FF, vp, vm, vF, vv and the NaN flag
#define UF3_NEB_BAD_FORCE 1                 // NebImage::bad
#define UF3_NEB_BAD_TANGENT 2

struct NebBand {                            // one band's optimiser state (device)
    FireState fire;
    double spring, crit_last;              // crit_last: the criterion at the last evaluation while running
    int status, climbing;                  // climbing: the image (index within the band) that climbed at that evaluation, or -1
    int frame0, n_img;                     // the band's first frame and its number of images
};

struct NebImage {                           // what k_neb_force leaves of one image for k_neb_band
    double cp, cm, gv, gg, vv;             // g = F + cp t+ + cm t-; g.v, |g|^2, |v|^2 over the image
    int bad, pad;
};

struct NebCoef {                            // what k_neb_move needs of its band's decision in this step
    FireStep k;
    int move, pad;
};

struct NebChunkArgs {                       // k_neb_partial and k_neb_force
    const double *pos, *frc, *vel;         // [N][3]: the coordinates the band lives in (a cell band: q), the evaluator's forces,
                                           // the velocities
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
    // cell bands only
    const double *virials;                 // [n_frames][6]
    const double *D, *vc;                  // [n_frames][9]: the deformations and the velocities of Y
    const double *kappa;                   // [n_bands]
    double *fq;                            // [N][3]: F D^T
    double *G, *D_ev, *vc_ev;              // [n_frames][9]: the cell force, and D and vc at this evaluation (k_neb_move's input)
    double *gc;                            // [n_frames][9]: the cell part of g (0 on end points and images without a tangent)
};

__device__ __forceinline__ double neb_dot(const double a[3], const double b[3]) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// t+ and t- of atom i of an interior image whose frame holds na atoms (the images of a band are consecutive frames)
__device__ __forceinline__ void neb_diffs(const double *pos, long long i, long long na, double p[3], double m[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double x = pos[3 * i + k];
        p[k] = pos[3 * (i + na) + k] - x;
        m[k] = x - pos[3 * (i - na) + k];
    }
}

// entry k of the cell parts of t+ and t- of interior image f: Y = kappa D, as stored
__device__ __forceinline__ void neb_cell_diffs(const double *D, int f, int k, double kap, double &p, double &m) {
    const double y = kap * D[9 * f + k];
    p = kap * D[9 * (f + 1) + k] - y;
    m = y - kap * D[9 * (f - 1) + k];
}

// one atom's ten dot products among {t+, t-, F, v} (f2 = |F|^2)
__device__ __forceinline__ void neb_dots(const double p[3], const double m[3], const double F[3], double f2, const double v[3],
                                         double *s) {
    s[0] = neb_dot(p, p);
    s[1] = neb_dot(p, m);
    s[2] = neb_dot(m, m);
    s[3] = neb_dot(F, p);
    s[4] = neb_dot(F, m);
    s[5] = f2;
    s[6] = neb_dot(v, p);
    s[7] = neb_dot(v, m);
    s[8] = neb_dot(v, F);
    s[9] = neb_dot(v, v);
}

template <bool CELL>
__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_neb_partial(NebChunkArgs A) {
    __shared__ double lds[UF3_NEB_NSUM * UF3_RELAX_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const int f = A.blk_frame[b];
    const int bd = A.frame_band[f];
    const NebBand *B = A.bands + bd;
    if (!A.all && B->status != UF3_RELAX_RUNNING) return;
    const bool interior = f > B->frame0 && f < B->frame0 + B->n_img - 1;
    double D[9];
    if constexpr (CELL) {
#pragma unroll
        for (int k = 0; k < 9; k++) D[k] = A.D[9 * f + k];
        if (b == A.frame_blk[f] && t == 0) {            // one writer per image
            double G[9];
            relax_cell_force(D, A.virials + 6 * f, A.kappa[bd], G);
            for (int k = 0; k < 9; k++) { A.G[9 * f + k] = G[k]; A.D_ev[9 * f + k] = D[k]; A.vc_ev[9 * f + k] = A.vc[9 * f + k]; }
        }
    }
    double s[UF3_NEB_NSUM];
#pragma unroll
    for (int k = 0; k < UF3_NEB_NSUM; k++) s[k] = 0.0;
    if (t < A.blk_n[b]) {
        const long long i = A.blk_lo[b] + t;
        double F[3];
#pragma unroll
        for (int k = 0; k < 3; k++) F[k] = A.frc[3 * i + k];
        double f2 = neb_dot(F, F);
        bool fin = isfinite(f2);
        if constexpr (CELL) {                           // the force on q, F D^T, in the place of F
            double Fx[3];
#pragma unroll
            for (int k = 0; k < 3; k++) Fx[k] = F[k];
            relax_g(Fx, D, true, false, F);
#pragma unroll
            for (int k = 0; k < 3; k++) A.fq[3 * i + k] = F[k];
            f2 = neb_dot(F, F);
            fin = fin && isfinite(f2);
        }
        s[10] = fin ? 0.0 : __builtin_nan("");
        if (interior && !(A.fixed && A.fixed[i])) {
            double p[3], m[3], v[3];
            neb_diffs(A.pos, i, A.offsets[f + 1] - A.offsets[f], p, m);
#pragma unroll
            for (int k = 0; k < 3; k++) v[k] = A.vel[3 * i + k];
            neb_dots(p, m, F, f2, v, s);
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

// image f's sums: its chunks' partials in a strided pass, then the tree (the same bits in every chunk of the image)
__device__ __forceinline__ void neb_image_sums(const NebChunkArgs &A, int f, double (&s)[UF3_NEB_NSUM], double *lds) {
#pragma unroll
    for (int k = 0; k < UF3_NEB_NSUM; k++) s[k] = 0.0;
    for (int c = A.frame_blk[f] + threadIdx.x; c < A.frame_blk[f + 1]; c += UF3_RELAX_THREADS) {
#pragma unroll
        for (int k = 0; k < UF3_NEB_NSUM - 1; k++) s[k] += A.partial[UF3_NEB_NSUM * c + k];
        s[10] = relax_nanmax(s[10], A.partial[UF3_NEB_NSUM * c + 10]);
    }
    relax_block_reduce<UF3_NEB_NSUM>(s, lds);
}

// the improved tangent's weights of interior image f from the energies: tau = wp t+ + wm t-.  (wm before wp throughout: the
// compiler orders the two products of F . tau^ by it, and which of them it contracts into the sum decides the last bit)
__device__ __forceinline__ void neb_tangent_weights(const double *energies, int f, double &wm, double &wp) {
    const double Em = energies[f - 1], E0 = energies[f], Ep = energies[f + 1];
    if (Ep > E0 && E0 > Em) { wm = 0.0; wp = 1.0; }
    else if (Ep < E0 && E0 < Em) { wm = 1.0; wp = 0.0; }
    else {
        const double dp = fabs(Ep - E0), dm = fabs(Em - E0);
        const double dmax = dp > dm ? dp : dm, dmin = dp > dm ? dm : dp;
        if (Ep > Em) { wm = dmin; wp = dmax; } else { wm = dmax; wp = dmin; }
    }
}

// an interior image from its sums and tangent weights: c+ and c- of g = F + c+ t+ + c- t- (the spring along the tangent and
// F's part across it, or F turned round along it on the climbing image), the tangent's flag in bad, and, from the image's one
// writer (out not null), what k_neb_band sums.  j: the image's index within band B
__device__ __forceinline__ void neb_image(const double *s, double wp, double wm, const double *energies, const NebBand *B, int climb,
                                          int j, int &bad, double &cp, double &cm, NebImage *out) {
    const double pp = s[0], pm = s[1], mm = s[2], Fp = s[3], Fm = s[4], FF = s[5], vp = s[6], vm = s[7], vF = s[8], vv = s[9];
    const double tau2 = wp * wp * pp + 2.0 * wp * wm * pm + wm * wm * mm;
    if (!(tau2 > 0.0) || !isfinite(tau2)) bad |= UF3_NEB_BAD_TANGENT;
    const double itau = 1.0 / sqrt(tau2);
    const double Ft = (wp * Fp + wm * Fm) * itau;                       // F . tau^
    // (the climbing image is looked up here, between F . tau^ and c: its loop keeps the compiler from contracting across it,
    // and the band's bits depend on that)
    const bool climbs = neb_climbing(energies, B, climb) == j;
    const double c = climbs ? -2.0 * Ft : B->spring * (sqrt(pp) - sqrt(mm)) - Ft;
    cm = c * wm * itau; cp = c * wp * itau;                             // (cm first, for the same reason as wm)
    if (out) {
        NebImage I;
        I.cp = cp; I.cm = cm;
        I.gv = vF + cp * vp + cm * vm;
        I.gg = FF + cp * cp * pp + cm * cm * mm + 2.0 * (cp * Fp + cm * Fm + cp * cm * pm);
        I.vv = vv;
        I.bad = bad; I.pad = 0;
        *out = I;
    }
}

template <bool CELL>
__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_neb_force(NebChunkArgs A) {
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
    neb_image_sums(A, f, s, lds);
    int bad = (s[10] != s[10]) ? UF3_NEB_BAD_FORCE : 0;
    const double kap = CELL ? A.kappa[bd] : 0.0;
    const double *G = CELL ? A.G + 9 * f : nullptr;
    if constexpr (CELL) {
        bool gfin = true;
        for (int k = 0; k < 9; k++) gfin = gfin && isfinite(G[k]);
        if (!gfin) bad = UF3_NEB_BAD_FORCE;
    }
    const long long i = A.blk_lo[b] + t;
    const bool mine = t < A.blk_n[b];
    if (!interior) {
        if (lead) {
            NebImage I = {0.0, 0.0, 0.0, 0.0, 0.0, bad, 0};
            A.img[f] = I;
            if constexpr (CELL)
                for (int k = 0; k < 9; k++) A.gc[9 * f + k] = 0.0;
        }
        if (mine) {
#pragma unroll
            for (int k = 0; k < 3; k++) A.g[3 * i + k] = 0.0;
        }
        return;
    }
    if constexpr (CELL) {
        // the nine cell entries, once per image, after the chunk sums, entry by entry (every thread: the same bits)
        for (int k = 0; k < 9; k++) {
            double p, m;
            neb_cell_diffs(A.D, f, k, kap, p, m);
            const double Gk = G[k], vk = A.vc[9 * f + k];
            s[0] += p * p; s[1] += p * m; s[2] += m * m;
            s[3] += Gk * p; s[4] += Gk * m; s[5] += Gk * Gk;
            s[6] += vk * p; s[7] += vk * m; s[8] += vk * Gk; s[9] += vk * vk;
        }
    }
    double wm, wp;
    neb_tangent_weights(A.energies, f, wm, wp);
    double cp, cm;
    neb_image(s, wp, wm, A.energies, B, A.climb, f - B->frame0, bad, cp, cm, lead ? A.img + f : nullptr);
    const bool tangent = !(bad & UF3_NEB_BAD_TANGENT);          // (no tangent, no NEB force: g = 0, the band freezes)
    double m2[1] = {0.0};
    if (mine) {
        double g[3] = {0.0, 0.0, 0.0};
        if (tangent && !(A.fixed && A.fixed[i])) {
            const double *F = CELL ? A.fq : A.frc;
            double p[3], m[3];
            neb_diffs(A.pos, i, A.offsets[f + 1] - A.offsets[f], p, m);
#pragma unroll
            for (int k = 0; k < 3; k++) g[k] = F[3 * i + k] + cp * p[k] + cm * m[k];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) A.g[3 * i + k] = g[k];
        m2[0] = neb_dot(g, g);
    }
    if constexpr (CELL) {
        if (first && t < 3) {                           // row t of the cell part of g
            double r2 = 0.0;
            for (int k = 3 * t; k < 3 * t + 3; k++) {
                double p, m, gk = 0.0;
                neb_cell_diffs(A.D, f, k, kap, p, m);
                if (tangent) gk = G[k] + cp * p + cm * m;
                A.gc[9 * f + k] = gk;
                r2 += gk * gk;
            }
            m2[0] = relax_nanmax(m2[0], r2);
        }
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
                K->k = fire_step(B->fire, GV, GG, VV, A.dt0, A.dt_max, A.maxstep);
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
    // cell bands only
    double *q;                             // [N][3]
    double *D, *vc, *cells;                // [n_frames][9]
    const double *gc, *D_ev, *vc_ev;       // [n_frames][9]
    const double *kappa;                   // [n_bands]
    const long long *offsets;              // [n_frames + 1]
};

template <bool CELL>
__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_neb_move(NebMoveArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const int f = A.frame_of[i], bd = A.frame_band[f];
    const NebCoef *K = A.coef + bd;
    const NebBand *B = A.bands + bd;
    if (!K->move || f == B->frame0 || f == B->frame0 + B->n_img - 1 || (A.fixed && A.fixed[i])) return;
    const FireStep step = K->k;
    double Dn[9], vn[9];
    if constexpr (CELL) {
        const double kap = A.kappa[bd];
#pragma unroll
        for (int k = 0; k < 9; k++) {
            const double g = A.gc[9 * f + k];
            double dr;
            vn[k] = fire_kick(step, A.vc_ev[9 * f + k], g, dr);
            Dn[k] = A.D_ev[9 * f + k] + dr / kap;
        }
    }
    double *X = CELL ? A.q : A.pos;                     // the coordinates that move
    double x[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double g = A.g[3 * i + k];
        double dr;
        A.vel[3 * i + k] = fire_kick(step, A.vel[3 * i + k], g, dr);
        x[k] = X[3 * i + k] + dr;
        X[3 * i + k] = x[k];
    }
    if constexpr (CELL) {
#pragma unroll
        for (int k = 0; k < 3; k++) A.pos[3 * i + k] = x[0] * Dn[k] + x[1] * Dn[3 + k] + x[2] * Dn[6 + k];
        if (i == A.offsets[f]) {                        // one writer per image; C0 is the cell of the band's first image
            const double *C0 = A.cells + 9 * (size_t)B->frame0;
#pragma unroll
            for (int k = 0; k < 9; k++) { A.D[9 * f + k] = Dn[k]; A.vc[9 * f + k] = vn[k]; }
            for (int r = 0; r < 3; r++)
                for (int j = 0; j < 3; j++)
                    A.cells[9 * f + 3 * r + j] = C0[3 * r] * Dn[j] + C0[3 * r + 1] * Dn[3 + j] + C0[3 * r + 2] * Dn[6 + j];
        }
    }
}
