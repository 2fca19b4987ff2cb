// uf3_relax.h -- batched structure relaxation on the device (uf3_relax_*, include/uf3_hip.h): FIRE in ASE's formulation, every
// frame its own optimiser, optionally with the cell as extra degrees of freedom (relax_fmax's generalised coordinates: ASE's
// UnitCellFilter with cell_factor = n).  The forces come from the evaluator (eval_impl) before the three launches of a step:
//
//   k_relax_partial  one 256-thread workgroup per chunk of <= 256 atoms of one frame (chunks never straddle frames): the chunk's
//                    g.v, |g|^2, |v|^2 and the largest per-atom |F_i|^2 (NaN when a force is not finite)
//   k_relax_frame    one workgroup per frame: the frame's partials in a fixed order, then FIRE's state machine on lane 0 (the cell
//                    rows' terms, the convergence test, the mixing coefficients, the trust radius, the new D and cell)
//   k_relax_move     one thread per atom: mix, kick, scale, move (cell frames: q += dr, x = q D)
//
// Generalised coordinates of a cell frame: x = q D (row vectors), cell = cell0 D, cell coordinates Y = n D.  Force on q: F D^T;
// force on Y: G = -D^-T W / n, W the 3x3 strain derivative of uf3_eval_virial.  Nothing here uses atomics: the per-frame sums
// depend on the frame alone (chunks start at the frame's first atom), never on the batch around it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define UF3_RELAX_THREADS 256              // chunk size and workgroup of every relax kernel (the sums' order depends on it)
#define UF3_RELAX_RUNNING 0
#define UF3_RELAX_CONVERGED 1
#define UF3_RELAX_NONFINITE 2

// FIRE's constants (ASE's defaults)
#define UF3_FIRE_NMIN 5
#define UF3_FIRE_FINC 1.1
#define UF3_FIRE_FDEC 0.5
#define UF3_FIRE_ASTART 0.1
#define UF3_FIRE_FA 0.99

struct FireState {                          // one optimiser's FIRE state: a frame here, a band in uf3_neb.h
    double dt, alpha;
    long long steps;
    int n_pos, first;
};

struct FireStep {                           // one move as FIRE decided it: v' = (a v + b g) + dt g; dr = dt v' (* s when the trust
    double a, b, dt, s;                    // radius cuts: scale)
    int scale, pad;
};

// FIRE's state machine, the only copy: the decision for one optimiser's whole vector from its g.v, |g|^2 and |v|^2; S advances
__device__ __forceinline__ FireStep fire_step(FireState &S, double GV, double GG, double VV, double dt0, double dt_max,
                                              double maxstep) {
    double a = 1.0, b = 0.0, dt = S.first ? dt0 : S.dt, alpha = S.alpha;
    int n_pos = S.n_pos;
    if (!S.first) {
        if (GV > 0.0) {
            a = 1.0 - alpha;
            b = alpha * sqrt(VV) / sqrt(GG);
            if (n_pos > UF3_FIRE_NMIN) { dt = fmin(dt * UF3_FIRE_FINC, dt_max); alpha *= UF3_FIRE_FA; }
            n_pos += 1;
        } else {
            a = 0.0; b = 0.0;
            alpha = UF3_FIRE_ASTART; dt *= UF3_FIRE_FDEC; n_pos = 0;
        }
    }
    // |v'|^2 of v' = a v + (b + dt) g from the sums
    const double c = b + dt;
    const double v2 = fmax(a * a * VV + 2.0 * a * c * GV + c * c * GG, 0.0);
    const double drn = dt * sqrt(v2);
    const int scale = drn > maxstep;
    S.dt = dt; S.alpha = alpha; S.n_pos = n_pos; S.first = 0; S.steps += 1;
    const FireStep K = {a, b, dt, scale ? maxstep / drn : 1.0, scale, 0};
    return K;
}

// the kick of one degree of freedom, the only copy: its new velocity, and in dr its move
__device__ __forceinline__ double fire_kick(const FireStep &K, double v, double g, double &dr) {
    const double vn = (K.a * v + K.b * g) + K.dt * g;
    dr = K.dt * vn;
    if (K.scale) dr *= K.s;
    return vn;
}

struct RelaxFrame {                         // one frame's optimiser state (device)
    FireState fire;
    double e_last, fmax_last;              // energy and criterion at the last evaluation while running
    double D[9], cell0[9], vc[9];          // deformation (cell = cell0 D), reference cell, velocity of Y = n D
    int status, cellf;                     // cellf: the cell is a degree of freedom (relax_cell, periodic along all axes)
};

struct RelaxCoef {                          // what k_relax_move needs of its frame's decision in this step
    FireStep k;
    double Dold[9], Dnew[9];               // D at the evaluation (g = F Dold^T) and after the step (x = q Dnew)
    int move, cellf;
};

struct RelaxPartialArgs {
    const double *frc, *vel;               // [N][3]
    const uint8_t *fixed;                  // [N] or null
    const int *blk_frame;                  // [n_blocks]
    const long long *blk_lo;               // [n_blocks]: the chunk's first atom
    const int *blk_n;                      // [n_blocks]: atoms in the chunk (<= 256)
    const RelaxFrame *st;
    double *partial;                       // [n_blocks][4]
};

__device__ __forceinline__ double relax_nanmax(double x, double y) { return (x != x || y != y) ? (x + y) : (x > y ? x : y); }

// NS - 1 sums and one NaN-sticky max (the last) over a 256-wide workgroup in a fixed order -> every lane's s[] (uf3_neb.h's too)
template <int NS>
__device__ __forceinline__ void relax_block_reduce(double (&s)[NS], double *lds) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NS; k++) lds[k * UF3_RELAX_THREADS + t] = s[k];
    __syncthreads();
    for (int h = UF3_RELAX_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) {
#pragma unroll
            for (int k = 0; k < NS - 1; k++) lds[k * UF3_RELAX_THREADS + t] += lds[k * UF3_RELAX_THREADS + t + h];
            lds[(NS - 1) * UF3_RELAX_THREADS + t] =
                relax_nanmax(lds[(NS - 1) * UF3_RELAX_THREADS + t], lds[(NS - 1) * UF3_RELAX_THREADS + t + h]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < NS; k++) s[k] = lds[k * UF3_RELAX_THREADS];
    __syncthreads();                        // (the next reduction writes lds again)
}

// g = F D^T of a cell frame (row vector times D transposed), else F; zero for a fixed atom
__device__ __forceinline__ void relax_g(const double F[3], const double *D, bool cellf, bool fixed, double g[3]) {
#pragma unroll
    for (int k = 0; k < 3; k++)
        g[k] = fixed ? 0.0 : (cellf ? F[0] * D[3 * k] + F[1] * D[3 * k + 1] + F[2] * D[3 * k + 2] : F[k]);
}

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_relax_partial(RelaxPartialArgs A) {
    __shared__ double lds[4 * UF3_RELAX_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    const RelaxFrame *S = A.st + A.blk_frame[b];
    if (S->status != UF3_RELAX_RUNNING) return;         // (the frame kernel reads no partial of a frame that is not running)
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    if (t < A.blk_n[b]) {
        const long long i = A.blk_lo[b] + t;
        const bool fx = A.fixed && A.fixed[i];
        double F[3], v[3], g[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { F[k] = A.frc[3 * i + k]; v[k] = A.vel[3 * i + k]; }
        relax_g(F, S->D, S->cellf != 0, fx, g);
        s[0] = g[0] * v[0] + g[1] * v[1] + g[2] * v[2];
        s[1] = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
        s[2] = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
        const double f2 = F[0] * F[0] + F[1] * F[1] + F[2] * F[2];
        s[3] = !isfinite(f2) ? __builtin_nan("") : (fx ? 0.0 : f2);
    }
    relax_block_reduce(s, lds);
    if (t == 0) {
#pragma unroll
        for (int k = 0; k < 4; k++) A.partial[4 * b + k] = s[k];
    }
}

struct RelaxFrameArgs {
    const double *partial;                 // [n_blocks][4]
    const int *frame_blk;                  // [n_frames + 1]: the frame's chunks
    const long long *offsets;              // [n_frames + 1]
    const double *energies, *virials;      // [n_frames], [n_frames][6] (null: no cell frame in the batch)
    RelaxFrame *st;
    RelaxCoef *coef;
    double *cells;                         // [n_frames][9]: cell0 D, written for cell frames
    double *rec;                           // this step's record row [n_frames][2] (E, fmax) or null
    double fmax, dt0, dt_max, maxstep;     // dt0: the time step of a frame's first move (later moves carry their own)
    int can_move;                          // 0 on the run's last evaluation: the convergence test only
};

__host__ __device__ __forceinline__ void relax_inv3(const double *m, double *r) {
    const double c00 = m[4] * m[8] - m[5] * m[7], c01 = m[5] * m[6] - m[3] * m[8], c02 = m[3] * m[7] - m[4] * m[6];
    const double id = 1.0 / (m[0] * c00 + m[1] * c01 + m[2] * c02);
    r[0] = c00 * id; r[1] = (m[2] * m[7] - m[1] * m[8]) * id; r[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    r[3] = c01 * id; r[4] = (m[0] * m[8] - m[2] * m[6]) * id; r[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    r[6] = c02 * id; r[7] = (m[1] * m[6] - m[0] * m[7]) * id; r[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

// the force on the cell coordinates Y = kappa D: G = -D^-T W / kappa, W the strain derivative as uf3_eval_virial's six numbers
// (not finite for a singular D)
__device__ __forceinline__ void relax_cell_force(const double *D, const double *v, double kappa, double G[9]) {
    const double W[9] = {v[0], v[5], v[4], v[5], v[1], v[3], v[4], v[3], v[2]};
    double Di[9];
    relax_inv3(D, Di);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) G[3 * i + j] = -(Di[i] * W[j] + Di[3 + i] * W[3 + j] + Di[6 + i] * W[6 + j]) / kappa;
}

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_relax_frame(RelaxFrameArgs A) {
    __shared__ double lds[4 * UF3_RELAX_THREADS];
    const int f = blockIdx.x, t = threadIdx.x;
    RelaxFrame *S = A.st + f;
    RelaxCoef *K = A.coef + f;
    const int status0 = S->status;
    if (status0 == UF3_RELAX_RUNNING) {
        double s[4] = {0.0, 0.0, 0.0, 0.0};
        for (int b = A.frame_blk[f] + t; b < A.frame_blk[f + 1]; b += UF3_RELAX_THREADS) {
#pragma unroll
            for (int k = 0; k < 3; k++) s[k] += A.partial[4 * b + k];
            s[3] = relax_nanmax(s[3], A.partial[4 * b + 3]);
        }
        relax_block_reduce(s, lds);
        if (t == 0) {
            const bool cellf = S->cellf != 0;
            const double n = (double)(A.offsets[f + 1] - A.offsets[f]);
            const double E = A.energies[f];
            bool finite = isfinite(E) && isfinite(s[0]) && isfinite(s[1]) && isfinite(s[2]) && isfinite(s[3]);
            double G[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, D[9];
#pragma unroll
            for (int k = 0; k < 9; k++) D[k] = S->D[k];
            if (cellf) {
                relax_cell_force(D, A.virials + 6 * f, n, G);
                for (int k = 0; k < 9; k++) finite = finite && isfinite(G[k]);
            }
            double crit = sqrt(s[3]);
            for (int i = 0; i < 3; i++) crit = fmax(crit, sqrt(G[3 * i] * G[3 * i] + G[3 * i + 1] * G[3 * i + 1] + G[3 * i + 2] * G[3 * i + 2]));
            S->e_last = E;
            S->fmax_last = finite ? crit : __builtin_nan("");
            int move = 0;
            if (!finite) {
                S->status = UF3_RELAX_NONFINITE;
            } else if (crit < A.fmax) {
                S->status = UF3_RELAX_CONVERGED;
            } else if (A.can_move) {
                double GV = s[0], GG = s[1], VV = s[2];
                for (int k = 0; k < 9; k++) { GV += G[k] * S->vc[k]; GG += G[k] * G[k]; VV += S->vc[k] * S->vc[k]; }
                const FireStep step = fire_step(S->fire, GV, GG, VV, A.dt0, A.dt_max, A.maxstep);
                if (cellf) {
                    for (int k = 0; k < 9; k++) {
                        double dr;
                        S->vc[k] = fire_kick(step, S->vc[k], G[k], dr);
                        S->D[k] = D[k] + dr / n;
                    }
                    for (int i = 0; i < 3; i++)
                        for (int j = 0; j < 3; j++)
                            A.cells[9 * f + 3 * i + j] = S->cell0[3 * i] * S->D[j] + S->cell0[3 * i + 1] * S->D[3 + j] +
                                                         S->cell0[3 * i + 2] * S->D[6 + j];
                }
                K->k = step;
                for (int k = 0; k < 9; k++) { K->Dold[k] = D[k]; K->Dnew[k] = S->D[k]; }
                move = 1;
            }
            K->move = move;
            K->cellf = S->cellf;
        }
    } else if (t == 0) {
        K->move = 0;
    }
    if (A.rec && t == 0) {
        A.rec[2 * f] = S->e_last;
        A.rec[2 * f + 1] = S->fmax_last;
    }
}

struct RelaxMoveArgs {
    double *pos, *vel, *q;                 // [N][3]; q: cell runs only (null otherwise)
    const double *frc;
    const uint8_t *fixed;
    const int *frame_of;                   // [N]
    const RelaxCoef *coef;
    long long n;
};

__global__ void __launch_bounds__(UF3_RELAX_THREADS) k_relax_move(RelaxMoveArgs A) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= A.n) return;
    const RelaxCoef *K = A.coef + A.frame_of[i];
    if (!K->move || (A.fixed && A.fixed[i])) return;
    const bool cellf = K->cellf != 0;
    double F[3], g[3], dr[3];
#pragma unroll
    for (int k = 0; k < 3; k++) F[k] = A.frc[3 * i + k];
    relax_g(F, K->Dold, cellf, false, g);
    const FireStep step = K->k;
#pragma unroll
    for (int k = 0; k < 3; k++) A.vel[3 * i + k] = fire_kick(step, A.vel[3 * i + k], g[k], dr[k]);
    if (cellf) {
        double q[3];
#pragma unroll
        for (int k = 0; k < 3; k++) { q[k] = A.q[3 * i + k] + dr[k]; A.q[3 * i + k] = q[k]; }
        const double *D = K->Dnew;
#pragma unroll
        for (int k = 0; k < 3; k++) A.pos[3 * i + k] = q[0] * D[k] + q[1] * D[3 + k] + q[2] * D[6 + k];
    } else {
#pragma unroll
        for (int k = 0; k < 3; k++) A.pos[3 * i + k] += dr[k];
    }
}
