// uf3_md.h -- device-resident molecular dynamics (uf3_md_*, include/uf3_hip.h): the integrator, its random numbers and its
// per-frame sums.  The forces come from the evaluator (eval_impl) between two launches of k_md_step.
//
//   md_philox        Philox4x32-10 (Salmon et al., SC'11): counter (atom, step lo, step hi, draw), key (seed lo, seed hi)
//   k_md_step        one fused launch between two force calls: closing half-kick of step t (+ the atom's kinetic terms on a
//                    thermo step: md_store_kin), opening half-kick of step t + 1, drift; with LANGEVIN the drift is BAOAB's A-O-A
//   k_md_thermo      one workgroup per frame: the per-atom kinetic terms summed in a fixed order (md_kin_sum), one thermo record
//                    (md_store_kin and md_kin_sum are k_npt_move's and k_npt_thermo's too, uf3_npt.h: one copy of each)
//   k_md_init_velocities   Maxwell-Boltzmann draws, one thread per atom
//   k_md_init_com    one workgroup per frame: centre-of-mass velocity removed, optional rescale to the exact temperature (3N
//                    degrees of freedom)
//   k_philox_debug   the generator on caller-given counters and keys (uf3_philox_debug, tests)
//   k_md_wrap        opt-in periodic wrapping (uf3_md_set_wrap), one thread per atom: pos -= n . cell, img += n with n = floor of
//                    the fractional coordinate on periodic axes; k_md_unwrap forms pos + img . cell (or folds it back into pos)
//   k_md_msd_partial, k_md_msd_frame   the mean-squared-displacement sums of one sample (uf3_md_run_msd): one workgroup per chunk
//                    of the drivers' chunk table, then one per frame that adds the chunks in their order
//
// Units: Angstrom, fs, amu, eV, K.  Nothing here uses atomics: the sums are thread-strided partial sums + a tree in LDS, whose
// order depends on the atom count alone, so thermo records repeat bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define UF3_MD_ACC 0.009648533215665327        // eV / (Angstrom amu) -> Angstrom / fs^2
#define UF3_MD_KE 103.64269652680505           // amu Angstrom^2 / fs^2 -> eV
#define UF3_MD_KB 8.617333262e-5               // eV / K
#define UF3_MD_THREADS 256                     // workgroup of the per-frame kernels (the sums' order depends on it)

__device__ __forceinline__ uint4 md_philox(uint4 ctr, uint2 key) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint32_t lo0 = M0 * ctr.x, hi0 = __umulhi(M0, ctr.x);
        const uint32_t lo1 = M1 * ctr.z, hi1 = __umulhi(M1, ctr.z);
        ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
        key.x += W0; key.y += W1;
    }
    return ctr;
}

// uniform in (0, 1) from two words: never 0, so the logarithm is safe
__device__ __forceinline__ double md_uniform(uint32_t hi, uint32_t lo) {
    const unsigned long long u = ((unsigned long long)hi << 32) | lo;
    return ((double)(u >> 11) + 0.5) * 0x1.0p-53;
}

// two standard normals from one Philox call (Box-Muller)
__device__ __forceinline__ double2 md_normal2(unsigned long long seed, long long atom, unsigned long long step, uint32_t draw) {
    const uint4 r = md_philox(make_uint4((uint32_t)atom, (uint32_t)step, (uint32_t)(step >> 32), draw),
                              make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    const double rad = sqrt(-2.0 * log(md_uniform(r.x, r.y))), phi = 2.0 * M_PI * md_uniform(r.z, r.w);
    double s, c;
    sincos(phi, &s, &c);
    return make_double2(rad * c, rad * s);
}

// three normals of one atom: draws d and d + 1, the fourth normal dropped
__device__ __forceinline__ void md_normal3(unsigned long long seed, long long atom, unsigned long long step, uint32_t d, double xi[3]) {
    const double2 a = md_normal2(seed, atom, step, d), b = md_normal2(seed, atom, step, d + 1);
    xi[0] = a.x; xi[1] = a.y; xi[2] = b.x;
}

struct MdStepArgs {
    double *pos, *vel;                 // [N][3]: positions (unwrapped), velocities at integer time t on entry
    const double *frc, *inv_m;         // [N][3] F(t), [N] 1 / mass
    double *kin;                       // [7][N] on a thermo step: 1/2 m v^2 | m v (x) v (Voigt), eV
    long long n;
    double dt;
    double c, kT;                      // LANGEVIN: exp(-gamma dt), k_B T (eV)
    unsigned long long seed, step;     // step: the absolute index of the step being opened (t)
    int close, open;                   // half-kick that closes step t | opening half-kick + drift of step t + 1
};

// the atom's kinetic terms of a thermo step, k_md_step's and k_npt_move's (uf3_npt.h): kin[7][n] = 1/2 m v^2 | m v (x) v (Voigt),
// eV.  The products stay (m * v_a) * v_b as written: the thermo records' bits follow the operand order.
__device__ __forceinline__ void md_store_kin(double *kin, long long n, long long i, double im, const double v[3]) {
    const double m = UF3_MD_KE / im;
    kin[i] = 0.5 * m * (v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    kin[n + i] = m * v[0] * v[0];
    kin[2 * n + i] = m * v[1] * v[1];
    kin[3 * n + i] = m * v[2] * v[2];
    kin[4 * n + i] = m * v[1] * v[2];
    kin[5 * n + i] = m * v[0] * v[2];
    kin[6 * n + i] = m * v[0] * v[1];
}

template <bool LANGEVIN, bool THERMO>
__global__ void __launch_bounds__(256) k_md_step(MdStepArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const double im = A.inv_m[i], h = 0.5 * A.dt, ka = im * UF3_MD_ACC;
    double v[3], a[3];
#pragma unroll
    for (int k = 0; k < 3; k++) { v[k] = A.vel[3 * i + k]; a[k] = A.frc[3 * i + k] * ka; }
    if (A.close) {
#pragma unroll
        for (int k = 0; k < 3; k++) v[k] += h * a[k];
    }
    if (THERMO) md_store_kin(A.kin, A.n, i, im, v);
    if (A.open) {
        double x[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { x[k] = A.pos[3 * i + k]; v[k] += h * a[k]; }
        if (LANGEVIN) {
            double xi[3];
            md_normal3(A.seed, i, A.step, 0, xi);
            const double sig = sqrt((1.0 - A.c * A.c) * A.kT * ka);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                x[k] += h * v[k];
                v[k] = A.c * v[k] + sig * xi[k];
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

// K partial sums of every thread of a UF3_MD_THREADS-wide workgroup -> lane 0's x[], in a fixed order
template <int K>
__device__ __forceinline__ void md_block_sum(double (&x)[K], double *lds) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; k++) lds[k * UF3_MD_THREADS + t] = x[k];
    __syncthreads();
    for (int s = UF3_MD_THREADS / 2; s > 0; s >>= 1) {
        if (t < s) {
#pragma unroll
            for (int k = 0; k < K; k++) lds[k * UF3_MD_THREADS + t] += lds[k * UF3_MD_THREADS + t + s];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < K; k++) x[k] = lds[k * UF3_MD_THREADS];
    __syncthreads();
}

// what k_md_thermo and k_npt_thermo (uf3_npt.h) start with: the kinetic terms a record of `width` doubles holds (1 of 7 when it
// is 2) summed over the atoms [lo, hi) of the workgroup's frame, in lane 0's s[]
__device__ __forceinline__ void md_kin_sum(const double *kin, long long n, long long lo, long long hi, int width, double (&s)[7]) {
    __shared__ double lds[7 * UF3_MD_THREADS];
    const int nk = width == 2 ? 1 : 7;
    for (long long i = lo + threadIdx.x; i < hi; i += UF3_MD_THREADS)
        for (int k = 0; k < nk; k++) s[k] += kin[k * n + i];
    md_block_sum<7>(s, lds);
}

// one record per frame: [PE, KE] or [PE, KE, W (6), K (6)]; rec = thermo + (record * n_frames + frame) * width
__global__ void __launch_bounds__(UF3_MD_THREADS) k_md_thermo(const double *kin, long long n, const int64_t *offsets,
                                                              const double *energies, const double *virials, double *rec_base,
                                                              int width) {
    const int f = blockIdx.x;
    double s[7] = {0, 0, 0, 0, 0, 0, 0};
    md_kin_sum(kin, n, offsets[f], offsets[f + 1], width, s);
    if (threadIdx.x == 0) {
        double *r = rec_base + (size_t)f * width;
        r[0] = energies[f];
        r[1] = s[0];
        if (width == 14)
            for (int k = 0; k < 6; k++) { r[2 + k] = virials[6 * f + k]; r[8 + k] = s[1 + k]; }
    }
}

// Maxwell-Boltzmann velocities (draws 2 and 3 of the step counter's stream: the steps use 0 and 1), one thread per atom
__global__ void __launch_bounds__(256) k_md_init_velocities(double *vel, const double *inv_m, long long n, double kT,
                                                            unsigned long long seed, unsigned long long step) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double xi[3];
    md_normal3(seed, i, step, 2, xi);
    const double sig = sqrt(kT * inv_m[i] * UF3_MD_ACC);
#pragma unroll
    for (int k = 0; k < 3; k++) vel[3 * i + k] = sig * xi[k];
}

// then, one workgroup per frame: the mass-weighted centre-of-mass velocity removed and (exact) a rescale to k_B T = 2 KE / 3N
// (separate from the draws: with the generator inlined the reductions spilled scalar registers)
__global__ void __launch_bounds__(UF3_MD_THREADS) k_md_init_com(double *vel, const double *inv_m, const int64_t *offsets, double kT,
                                                                int exact) {
    __shared__ double lds[4 * UF3_MD_THREADS];
    const int f = blockIdx.x;
    const long long lo = offsets[f], hi = offsets[f + 1];
    double p[4] = {0, 0, 0, 0};          // momentum (3) | mass
    for (long long i = lo + threadIdx.x; i < hi; i += UF3_MD_THREADS) {
        const double m = 1.0 / inv_m[i];
#pragma unroll
        for (int k = 0; k < 3; k++) p[k] += m * vel[3 * i + k];
        p[3] += m;
    }
    md_block_sum<4>(p, lds);
    double ke[1] = {0};
    for (long long i = lo + threadIdx.x; i < hi; i += UF3_MD_THREADS) {
        const double m = 1.0 / inv_m[i];
        double v2 = 0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double v = vel[3 * i + k] - p[k] / p[3];
            vel[3 * i + k] = v;
            v2 += v * v;
        }
        ke[0] += 0.5 * m * v2 * UF3_MD_KE;
    }
    if (!exact) return;
    md_block_sum<1>(ke, lds);
    if (!(ke[0] > 0.0)) return;
    const double scale = sqrt(kT * 1.5 * (double)(hi - lo) / ke[0]);
    for (long long i = lo + threadIdx.x; i < hi; i += UF3_MD_THREADS)
#pragma unroll
        for (int k = 0; k < 3; k++) vel[3 * i + k] *= scale;
}

// ---- periodic wrapping with image counts (uf3_md_set_wrap) ------------------------------------------------------------------
// A wrapping object stores pos and int32 img [N][3]; its position is pos + img . cell with the frame's CURRENT cell (rows are
// lattice vectors).  k_md_wrap runs in front of every neighbour-list build made for the object and in front of every evaluation
// on the rebuild-everything route, never between a list build and the steps that use those lists.  The invariant: an evaluation
// of a wrapping object never sees an atom farther outside its cell than that atom has moved since the last wrap -- at most
// skin / 2, or the constant-pressure limit -- so the evaluator's image-range rule and the nearest-image rule of the samplers
// (k_flux_lists) describe the same crystal.  A wrap rounds (pos - n . cell is not exact): a trajectory's last bits depend on
// where the lists were built.
struct MdWrapArgs {
    double *pos;                       // [N][3]
    int *img;                          // [N][3] image counts
    const double *cells;               // [n_frames][9] the current cells
    const unsigned char *pbc;          // [n_frames][3]
    const int *frame_of;               // [N]
    long long n;
    int *changed;                      // set to 1 by every thread that moved its atom (may be null)
};

// the cell's rows crossed pairwise, nrm[k] . a_k = vol: the fractional coordinate k of x is x . nrm[k] / vol (taken against the
// cell, not against edge lengths)
__device__ __forceinline__ double md_cell_normals(const double *c, double nrm[3][3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double *a = c + 3 * ((k + 1) % 3), *b = c + 3 * ((k + 2) % 3);
        nrm[k][0] = a[1] * b[2] - a[2] * b[1];
        nrm[k][1] = a[2] * b[0] - a[0] * b[2];
        nrm[k][2] = a[0] * b[1] - a[1] * b[0];
    }
    return c[0] * nrm[0][0] + c[1] * nrm[0][1] + c[2] * nrm[0][2];
}

// Idempotent up to one case: a coordinate that lands within an ulp of a face may be wrapped once more by the next call, which
// is harmless (it is the same crystal either way).  An atom inside the cell, a non-periodic axis and a non-periodic frame are
// left alone bit for bit.
__global__ void __launch_bounds__(256) k_md_wrap(MdWrapArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const int f = A.frame_of[i];
    const unsigned char *per = A.pbc + 3 * (size_t)f;
    if (!(per[0] | per[1] | per[2])) return;
    const double *c = A.cells + 9 * (size_t)f;
    double nrm[3][3], x[3];
    const double vol = md_cell_normals(c, nrm);
#pragma unroll
    for (int k = 0; k < 3; k++) x[k] = A.pos[3 * i + k];
    int n[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (!per[k]) continue;
        const double fl = floor((x[0] * nrm[k][0] + x[1] * nrm[k][1] + x[2] * nrm[k][2]) / vol);
        if (fabs(fl) <= 1.0e9) n[k] = (int)fl;          // (a singular cell gives no number: left alone)
    }
    if (!(n[0] | n[1] | n[2])) return;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        if (!n[k]) continue;
#pragma unroll
        for (int d = 0; d < 3; d++) x[d] = fma(-(double)n[k], c[3 * k + d], x[d]);
    }
#pragma unroll
    for (int k = 0; k < 3; k++) { A.pos[3 * i + k] = x[k]; A.img[3 * i + k] += n[k]; }
    if (A.changed) *A.changed = 1;
}

// pos + img . cell of one atom (img null: pos)
__device__ __forceinline__ void md_unwrapped(const double *pos, const int *img, const double *cells, const int *frame_of, long long i,
                                             double x[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++) x[k] = pos[3 * i + k];
    if (!img) return;
    const double *c = cells + 9 * (size_t)frame_of[i];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int n = img[3 * i + k];
        if (!n) continue;
#pragma unroll
        for (int d = 0; d < 3; d++) x[d] = fma((double)n, c[3 * k + d], x[d]);
    }
}

// out = pos + img . cell; fold: out is pos itself and img becomes zero (uf3_md_set_wrap off)
__global__ void __launch_bounds__(256) k_md_unwrap(MdWrapArgs A, double *out, int fold) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    double x[3];
    md_unwrapped(A.pos, A.img, A.cells, A.frame_of, i, x);
#pragma unroll
    for (int k = 0; k < 3; k++) out[3 * i + k] = x[k];
    if (fold && (A.img[3 * i] | A.img[3 * i + 1] | A.img[3 * i + 2])) {
        A.img[3 * i] = 0; A.img[3 * i + 1] = 0; A.img[3 * i + 2] = 0;
        if (A.changed) *A.changed = 1;
    }
}

// ---- mean-squared displacement (uf3_md_run_msd) -------------------------------------------------------------------------------
// One record per sample and frame of 4 S + 4 doubles, S the basis' species count: per species sum |dr|^2, sum dx, sum dy, sum dz
// over its atoms, dr = pos + img . cell - origin; then sum m dr (3) and sum m.  No atomics: the order of every sum depends on
// the atom counts alone, so records repeat bit for bit.  The reductions go species by species through 4 x 256 doubles of LDS.
struct MdMsdArgs {
    const double *pos, *origin, *mass, *cells;     // cells: [n_frames][9], read only when img is not null
    const int *img;                                // null: the object never wrapped
    const signed char *spec;                       // [N] species index (-1: outside the basis, in the mass sums only)
    const int *frame_of, *blk_n, *frame_blk;       // the chunk table
    const long long *blk_lo;
    double *partial;                               // [n_blocks][4 S + 4]
    double *rec;                                   // [n_frames][4 S + 4]
    int S;
};

__global__ void __launch_bounds__(UF3_MD_THREADS) k_md_msd_partial(MdMsdArgs A) {
    __shared__ double lds[4 * UF3_MD_THREADS];
    const int b = blockIdx.x, t = threadIdx.x, W = 4 * A.S + 4;
    double d[3] = {0.0, 0.0, 0.0}, m = 0.0;
    int s = -2;
    if (t < A.blk_n[b]) {
        const long long i = A.blk_lo[b] + t;
        md_unwrapped(A.pos, A.img, A.cells, A.frame_of, i, d);
#pragma unroll
        for (int k = 0; k < 3; k++) d[k] -= A.origin[3 * i + k];
        m = A.mass[i];
        s = A.spec[i];
    }
    const double d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
    for (int sp = 0; sp <= A.S; sp++) {
        const bool last = sp == A.S;               // the mass-weighted sums of every atom
        const bool mine = last ? s != -2 : s == sp;
        double q[4] = {0.0, 0.0, 0.0, 0.0};
        if (mine) {
            q[0] = last ? m * d[0] : d2; q[1] = last ? m * d[1] : d[0]; q[2] = last ? m * d[2] : d[1]; q[3] = last ? m : d[2];
        }
        md_block_sum<4>(q, lds);
        if (t == 0) {
#pragma unroll
            for (int k = 0; k < 4; k++) A.partial[(size_t)b * W + 4 * sp + k] = q[k];
        }
    }
}

// one workgroup per frame: entry k of the record is thread k's sum of the chunks' entries, in chunk order
__global__ void __launch_bounds__(64) k_md_msd_frame(MdMsdArgs A) {
    const int f = blockIdx.x, k = threadIdx.x, W = 4 * A.S + 4;
    if (k >= W) return;
    double s = 0.0;
    for (int b = A.frame_blk[f]; b < A.frame_blk[f + 1]; b++) s += A.partial[(size_t)b * W + k];
    A.rec[(size_t)f * W + k] = s;
}

__global__ void k_philox_debug(long long n, const uint4 *ctr, const uint2 *key, uint4 *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = md_philox(ctr[i], key[i]);
}
