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

__global__ void k_philox_debug(long long n, const uint4 *ctr, const uint2 *key, uint4 *out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = md_philox(ctr[i], key[i]);
}
