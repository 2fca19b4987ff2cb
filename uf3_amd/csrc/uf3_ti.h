// uf3_ti.h -- switching molecular dynamics between the model and an Einstein crystal (uf3_md_set_reference, uf3_md_run_switch,
// include/uf3_hip.h): H(lambda) = K + lambda U_uf3 + (1 - lambda) U_E with U_E = 1/2 sum k_i |x_i - x0_i|^2, lambda moving along
// a schedule, every frame its own lambda end points and temperature, and the switching work accumulated on the device.
//
//   k_ti_partial     one workgroup per chunk of the drivers' chunk table: the chunk's U_E, sum of spring forces, sum m, sum F_uf3
//                    and (friction with a fixed centre of mass) sum m dv of the O-step about to be opened, whose normals it draws
//                    again from the counters k_ti_step will use -- nothing is stored per atom
//   k_ti_frame       one workgroup per frame: the chunks added in their order, then lambda, D = U_uf3 - U_E, the work
//                    W += (lambda(j) - lambda(j - 1)) (D(j - 1) + D(j)) / 2 and the two projections' per-frame vectors
//   k_ti_step        one thread per atom, k_md_step's counterpart: closing half-kick (+ the kinetic terms on a record step),
//                    opening half-kick, drift (BAOAB's A-O-A with friction), with the mixed force
//                    F_i = lambda F_uf3,i - (1 - lambda) k_i (x_i - x0_i) - m_i (sum_j F_j / M) and the noise dv_i - sum m dv / M
//   k_ti_record      one workgroup per frame: [lambda, U_uf3, U_E, KE, W so far]
//
// As everywhere in uf3_md.h: no atomics, every sum in an order that depends on the atom counts alone, so work and records repeat
// bit for bit.  Both kernels that run after each force call launch on the chunk table (<= UF3_MD_THREADS atoms a chunk).
#pragma once
#include "uf3_md.h"

#define UF3_TI_PART 12                          // doubles of one chunk's partial sums (below)
#define UF3_TI_REC 5                            // doubles of one record

struct TiArgs {
    double *pos, *vel;                          // [N][3]
    const double *frc, *inv_m, *mass;           // [N][3] F_uf3 of pos, [N] 1 / mass, [N] mass
    double *kin;                                // [7][N] on a record step (md_store_kin)
    const double *x0, *spring;                  // [N][3] reference sites, [N] spring constants (eV / A^2)
    const int *frame_of, *blk_n, *frame_blk;    // the chunk table
    const long long *blk_lo;
    const double *energies;                     // [n_frames] U_uf3 of pos
    const double *kT, *lam_a, *lam_b;           // [n_frames] k_B T (eV), lambda at schedule value 0 and 1
    const double *sched;                        // [n_steps + 1] the run's schedule
    double *partial;                            // [n_blocks][UF3_TI_PART]: U_E, sum F_spring (3), sum m, sum F_uf3 (3), sum m dv (3), -
    double *lam, *ue, *d, *w;                   // [n_frames] of the current state: lambda, U_E, D; the work so far
    double *cf, *cn;                            // [n_frames][3] sum F_mixed / M (A amu^-1 eV), sum m dv / M (A / fs); zero when unused
    long long n;
    double dt, c;                               // c: exp(-gamma dt)
    unsigned long long seed, step;              // step: the absolute index of the step opened next
    long long j;                                // the state's index in the run, 0 .. n_steps
    int fix_com, noise;                         // noise: the state opens an O-step whose noise is projected
    int close, open;                            // k_ti_step: as MdStepArgs
};

// the O-step's sigma of atom i: dv = sigma xi is the term k_md_step adds
__device__ __forceinline__ double ti_sigma(const TiArgs &A, double im, int f) {
    return sqrt((1.0 - A.c * A.c) * A.kT[f] * (im * UF3_MD_ACC));
}

__global__ void __launch_bounds__(UF3_MD_THREADS) k_ti_partial(TiArgs A) {
    __shared__ double lds[4 * UF3_MD_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const bool mine = t < A.blk_n[b];
    const long long i = A.blk_lo[b] + (mine ? t : 0);
    double q[4] = {0.0, 0.0, 0.0, 0.0};
    if (mine) {
        const double ks = A.spring[i];
        double d2 = 0.0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double d = A.pos[3 * i + k] - A.x0[3 * i + k];
            d2 += d * d;
            q[1 + k] = -ks * d;
        }
        q[0] = 0.5 * ks * d2;
    }
    md_block_sum<4>(q, lds);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) A.partial[(size_t)b * UF3_TI_PART + k] = q[k];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = 0.0;
    if (mine) {
        q[0] = A.mass[i];
#pragma unroll
        for (int k = 0; k < 3; k++) q[1 + k] = A.frc[3 * i + k];
    }
    md_block_sum<4>(q, lds);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) A.partial[(size_t)b * UF3_TI_PART + 4 + k] = q[k];
    }
#pragma unroll
    for (int k = 0; k < 4; k++) q[k] = 0.0;
    if (A.noise) {                              // (the same for every thread of the launch)
        if (mine) {
            double xi[3];
            md_normal3(A.seed, i, A.step, 0, xi);
            const double ms = A.mass[i] * ti_sigma(A, A.inv_m[i], A.frame_of[i]);
#pragma unroll
            for (int k = 0; k < 3; k++) q[k] = ms * xi[k];
        }
        md_block_sum<4>(q, lds);
    }
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) A.partial[(size_t)b * UF3_TI_PART + 8 + k] = q[k];
    }
}

// thread k adds entry k of the frame's chunks in chunk order; thread 0 then closes the state
__global__ void __launch_bounds__(64) k_ti_frame(TiArgs A) {
    __shared__ double s[UF3_TI_PART];
    const int f = blockIdx.x, k = threadIdx.x;
    if (k < UF3_TI_PART) {
        double a = 0.0;
        for (int b = A.frame_blk[f]; b < A.frame_blk[f + 1]; b++) a += A.partial[(size_t)b * UF3_TI_PART + k];
        s[k] = a;
    }
    __syncthreads();
    if (k != 0) return;
    const double la = A.lam_a[f], lb = A.lam_b[f];
    const double lam = la + (lb - la) * A.sched[A.j], d = A.energies[f] - s[0];
    if (A.j == 0)
        A.w[f] = 0.0;
    else {
        const double before = la + (lb - la) * A.sched[A.j - 1];
        A.w[f] += (lam - before) * (0.5 * (A.d[f] + d));
    }
    A.lam[f] = lam; A.ue[f] = s[0]; A.d[f] = d;
#pragma unroll
    for (int x = 0; x < 3; x++) {
        A.cf[3 * f + x] = A.fix_com ? (lam * s[5 + x] + (1.0 - lam) * s[1 + x]) / s[4] : 0.0;
        A.cn[3 * f + x] = A.noise ? s[8 + x] / s[4] : 0.0;
    }
}

template <bool LANGEVIN, bool THERMO>
__global__ void __launch_bounds__(256) k_ti_step(TiArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const int f = A.frame_of[i];
    const double im = A.inv_m[i], h = 0.5 * A.dt, ka = im * UF3_MD_ACC, lam = A.lam[f], ks = (1.0 - lam) * A.spring[i];
    double x[3], v[3], a[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        x[k] = A.pos[3 * i + k]; v[k] = A.vel[3 * i + k];
        a[k] = (lam * A.frc[3 * i + k] - ks * (x[k] - A.x0[3 * i + k])) * ka - A.cf[3 * f + k] * UF3_MD_ACC;
    }
    if (A.close) {
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] += h * a[k];
    }
    if (THERMO) md_store_kin(A.kin, A.n, i, im, v);
    if (A.open) {
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] += h * a[k];
        if (LANGEVIN) {
            double xi[3];
            md_normal3(A.seed, i, A.step, 0, xi);
            const double sig = ti_sigma(A, im, f);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                x[k] += h * v[k];
                v[k] = A.c * v[k] + (sig * xi[k] - A.cn[3 * f + k]);
                x[k] += h * v[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) x[k] += A.dt * v[k];
        }
#pragma unroll
        for (int k = 0; k < 3; k++) A.pos[3 * i + k] = x[k];
    }
#pragma unroll
    for (int k = 0; k < 3; k++) A.vel[3 * i + k] = v[k];
}

// one record per frame of the state the launch before it closed: rec = records + (record * n_frames + frame) * UF3_TI_REC
__global__ void __launch_bounds__(UF3_MD_THREADS) k_ti_record(TiArgs A, const int64_t *offsets, double *rec_base) {
    const int f = blockIdx.x;
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    md_kin_sum(A.kin, A.n, offsets[f], offsets[f + 1], 2, s);
    if (threadIdx.x == 0) {
        double *r = rec_base + (size_t)f * UF3_TI_REC;
        r[0] = A.lam[f]; r[1] = A.energies[f]; r[2] = A.ue[f]; r[3] = s[0]; r[4] = A.w[f];
    }
}
