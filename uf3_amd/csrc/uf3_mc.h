// uf3_mc.h -- batched species-swap Monte Carlo on fixed positions (uf3_mc_*, include/uf3_hip.h): canonical swaps and
// semi-grand-canonical transmutations, every frame its own Markov chain.
//
//   mc_delta         E_touch(z') - E_touch(z) of one proposal: every energy term of the evaluator (k_eval) that contains a real
//                    atom of T = {i, j} (swap) or {i} (transmutation), for the new species minus for the old ones
//   k_mc_trials      one workgroup per frame runs a block of trials in one launch: proposal (Philox4x32-10 of uf3_md.h on
//                    (frame, trial lo, trial hi, 0)), mc_delta, Metropolis, records; the frame's species live in LDS
//   k_mc_delta       one workgroup per caller-given proposal: mc_delta alone, nothing applied
//
// The neighbour table depends on the geometry only (uf3_hip.hip builds it per object and per uf3_mc_set_positions): per atom the
// entries (real atom, squared distance) within the largest pair r_max and the entries (real atom, displacement, length) of the
// evaluator's 3-body range, both in the order of the reference supercell index -- the evaluator's list order among neighbours of one
// species.  Periodic images are separate entries with the same real atom; membership in T goes by the real atom.
//
// The terms, over the table:
//   centres t in T        the one-body term; every pair entry q of t -- the evaluator counts the bond from both ends, so an entry
//                         whose atom lies outside T stands for its mirror at that atom's centre as well (weight 2), and one inside T
//                         is met again from the other end (weight 1); every triplet (a < b) of t's 3-body entries
//   centres m not in T    each real atom among the 3-body entries of T's atoms, once (the table is symmetric: those are the
//                         centres whose lists mention T): the triplets (a < b) of m's entries with a or b in T
// A triplet's legs follow the evaluator: the entry with the lower (species, supercell index) is leg l.  Values come from
// trio_value and the pair splines' records (uf3_kernels.h / uf3_device.h); nothing about the splines is restated here.
//
// Sums: each lane adds its terms in list order, the wave's lanes through wave_sum (DPP), the waves' sums in wave order.  Which wave
// takes which centre depends on the table alone.  No atomics: the difference is a pure function of (positions, species, proposal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define UF3_MC_THREADS 256                 // workgroup of both kernels: 4 waves, a wave per affected centre at a time
#define UF3_MC_WAVES (UF3_MC_THREADS / 64)
#define UF3_MC_MAX_N3 512                  // most 3-body entries of one atom (the affected-centre list of a trial sits in LDS)
#define UF3_MC_MAX_ATOMS 49152             // most atoms of one frame (its species, one byte each, sit in LDS)
#define UF3_MC_BLOCK_TRIALS 1024           // trials per launch (tens of milliseconds at the measured time per trial)
#define UF3_MC_RUNNING 0
#define UF3_MC_NONFINITE 2

struct __attribute__((aligned(16))) McEnt2 { double s; int atom, pad; };              // squared distance | atom (index within the frame)
struct __attribute__((aligned(16))) McEnt3 { double dx, dy, dz, r; int atom, pad[3]; };

struct McTable {
    const long long *off2, *off3;          // [N + 1] first entry of each atom (batch-global atom index)
    const McEnt2 *ent2;
    const McEnt3 *ent3;
};

struct McModel {
    const BasisDev *B;
    const double *c1, *c2, *c3;
    int S, T;
};

struct McMove { int i, j, zi, zj; };       // atoms within the frame (j = -1: none) and their NEW species

__device__ __forceinline__ int mc_new_spec(const unsigned char *spec, const McMove &mv, int a) {
    return a == mv.i ? mv.zi : (a == mv.j ? mv.zj : (int)spec[a]);
}

// the pair term of species (sa, sb) at squared distance s, as k_eval's drain forms it
__device__ __forceinline__ double mc_pair_value(const McModel &M, int sa, int sb, double s) {
    const BasisDev *B = M.B;
    const int pidx = sa * UF3_MAX_SPECIES + sb;
    const int pi = B->pair_of[pidx];
    if (pi < 0) return 0.0;
    const double s_lo = B->pairs[pi].s_lo, s_hi = B->pairs[pi].s_hi;
    if (!((s > s_lo) & (s < s_hi))) return 0.0;
    const LegDev leg = B->pairs[pi].leg;
    const double d = sqrt(s);
    KnotRec kr;
    const int iv = load_interval<1>(load_const(&B->recs), leg, d, kr);
    double v[4];
    bspline4<false>(kr, d, v, nullptr);
    const double *cf = M.c2 + (B->pair_col[pidx] - M.S) + (iv - 3);
    double phi = 0.0;
    for (int q = 0; q < 4; q++) phi += cf[q] * v[q];
    return phi;
}

// the triplet of centre species sm with entries a < b (table order = supercell index order) of species sa, sb
__device__ __forceinline__ double mc_trio_value(const McModel &M, int sm, int sa, int sb, double ra, double rb, double rn) {
    const bool a_first = sa <= sb;
    const int s1 = a_first ? sa : sb, s2 = a_first ? sb : sa;
    const int trio = M.B->trio_of[(sm * UF3_MAX_SPECIES + s1) * UF3_MAX_SPECIES + s2];
    double val = 0.0, gr[3];
    if (!trio_value(M.B, M.c3, trio, a_first ? ra : rb, a_first ? rb : ra, rn, false, val, gr)) return 0.0;
    return val;
}

// one wave: the terms of centre m (index within the frame; `lo` its frame's first atom) that contain an atom of T, new minus old,
// summed over this lane's share.  whole: m itself is in T (every term of the centre counts).
__device__ __forceinline__ double mc_centre_delta(const McModel &M, const McTable &tb, const unsigned char *spec, long long lo, int m,
                                                  bool whole, const McMove &mv) {
    const int lane = threadIdx.x & 63;
    const int sm_o = spec[m], sm_n = mc_new_spec(spec, mv, m);
    double acc = 0.0;
    if (whole) {
        if (lane == 0) acc = M.c1[sm_n] - M.c1[sm_o];
        const long long b2 = tb.off2[lo + m];
        const int n2 = (int)(tb.off2[lo + m + 1] - b2);
        for (int q = lane; q < n2; q += 64) {
            const McEnt2 e = tb.ent2[b2 + q];
            const int so = spec[e.atom], sn = mc_new_spec(spec, mv, e.atom);
            const double w = (e.atom == mv.i || e.atom == mv.j) ? 1.0 : 2.0;
            acc += w * (mc_pair_value(M, sm_n, sn, e.s) - mc_pair_value(M, sm_o, so, e.s));
        }
    }
    if (M.T > 0) {
        const long long b3 = tb.off3[lo + m];
        const int n = (int)(tb.off3[lo + m + 1] - b3);
        const McEnt3 *ent = tb.ent3 + b3;
        const int n_pairs = n * (n - 1) / 2;
#pragma unroll 1
        for (int p = lane; p < n_pairs; p += 64) {
            // (pair index -> (aa < bb) as in k_eval)
            int bb = (int)((1.0f + __builtin_amdgcn_sqrtf(fmaf(8.0f, (float)p, 1.0f))) * 0.5f);
            bb -= (bb * (bb - 1) / 2 > p) ? 1 : 0;
            bb += ((bb + 1) * bb / 2 <= p) ? 1 : 0;
            const int aa = p - bb * (bb - 1) / 2;
            const int pa = ent[aa].atom, pb = ent[bb].atom;
            if (!whole && !(pa == mv.i || pa == mv.j || pb == mv.i || pb == mv.j)) continue;
            const McEnt3 ea = ent[aa], eb = ent[bb];
            const double rn = norm3_leg(eb.dx - ea.dx, eb.dy - ea.dy, eb.dz - ea.dz);
            acc += mc_trio_value(M, sm_n, mc_new_spec(spec, mv, pa), mc_new_spec(spec, mv, pb), ea.r, eb.r, rn) -
                   mc_trio_value(M, sm_o, spec[pa], spec[pb], ea.r, eb.r, rn);
        }
    }
    return acc;
}

struct McLds {
    int cand[2 + 2 * UF3_MC_MAX_N3];       // the affected centres of the proposal in flight (-1: none / met before)
    double wsum[UF3_MC_WAVES];
};

// the whole workgroup: E_touch(new) - E_touch(old) of the move, in every thread.  `spec`: the frame's species (LDS, as they are
// BEFORE the move).  Ends behind a barrier: the caller may change spec afterwards.
__device__ __forceinline__ double mc_delta(const McModel &M, const McTable &tb, const unsigned char *spec, McLds &L, long long lo,
                                           const McMove &mv) {
    const int t = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(t >> 6);
    int n_i = 0, n_j = 0;
    long long b_i = 0, b_j = 0;
    if (M.T > 0) {
        b_i = tb.off3[lo + mv.i]; n_i = (int)(tb.off3[lo + mv.i + 1] - b_i);
        if (mv.j >= 0) { b_j = tb.off3[lo + mv.j]; n_j = (int)(tb.off3[lo + mv.j + 1] - b_j); }
    }
    const int n_c = 2 + n_i + n_j;
    for (int k = t; k < n_c; k += UF3_MC_THREADS)
        L.cand[k] = k == 0 ? mv.i : (k == 1 ? (mv.j == mv.i ? -1 : mv.j) : (k - 2 < n_i ? tb.ent3[b_i + (k - 2)].atom : tb.ent3[b_j + (k - 2 - n_i)].atom));
    __syncthreads();
    // each real atom once: an entry is dropped when the atom is in T or stands earlier in the list
    bool drop[(2 + 2 * UF3_MC_MAX_N3 + UF3_MC_THREADS - 1) / UF3_MC_THREADS];
#pragma unroll
    for (int r = 0; r < (int)(sizeof(drop) / sizeof(drop[0])); r++) {
        const int k = 2 + t + r * UF3_MC_THREADS;
        drop[r] = false;
        if (k < n_c) {
            const int a = L.cand[k];
            bool d = a == mv.i || a == mv.j;
            for (int q = 2; q < k && !d; q++) d = L.cand[q] == a;
            drop[r] = d;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < (int)(sizeof(drop) / sizeof(drop[0])); r++)
        if (drop[r]) L.cand[2 + t + r * UF3_MC_THREADS] = -1;
    __syncthreads();
    double acc = 0.0;
    for (int k = wave; k < n_c; k += UF3_MC_WAVES) {
        const int m = __builtin_amdgcn_readfirstlane(L.cand[k]);
        if (m < 0) continue;
        acc += mc_centre_delta(M, tb, spec, lo, m, k < 2, mv);
    }
    acc = wave_sum(acc);
    if ((t & 63) == 0) L.wsum[wave] = acc;
    __syncthreads();
    double dE = L.wsum[0];
#pragma unroll
    for (int w = 1; w < UF3_MC_WAVES; w++) dE += L.wsum[w];
    __syncthreads();
    return dE;
}

struct McTrialArgs {
    McModel M;
    McTable tb;
    const long long *offsets;              // [n_frames + 1]
    int32_t *z;                            // [N] atomic numbers: the state
    const uint8_t *swappable;              // [N] or null (all)
    double *energy;                        // [n_frames] running energies
    long long *accepted, *trials;          // [n_frames]
    int *status;                           // [n_frames]
    const double *kT;                      // [n_frames] eV
    double mu[UF3_MAX_SPECIES];            // transmute: chemical potentials by species index, -inf: not allowed
    int s2z[UF3_MAX_SPECIES];              // species index -> atomic number
    int mode;                              // 0 swap, 1 transmute
    unsigned long long seed;
    unsigned long long t0;                 // absolute index of this launch's first trial
    int n_trials;                          // trials of this launch
    long long run_done;                    // trials of this run made by earlier launches
    long long rec_every;                   // 0: no records
    double *records;                       // [n_rec][n_frames][3 + S]
    int n_frames;
};

__global__ void __launch_bounds__(UF3_MC_THREADS) k_mc_trials(McTrialArgs A) {
    extern __shared__ __align__(16) unsigned char mc_spec[];
    __shared__ McLds L;
    __shared__ int count[UF3_MAX_SPECIES];
    const int f = blockIdx.x, t = threadIdx.x;
    const long long lo = A.offsets[f];
    const int n = (int)(A.offsets[f + 1] - lo);
    const BasisDev *B = A.M.B;
    if (A.status[f] != UF3_MC_RUNNING) return;
    if (t < UF3_MAX_SPECIES) count[t] = 0;
    for (int a = t; a < n; a += UF3_MC_THREADS) mc_spec[a] = (unsigned char)B->z2s[A.z[lo + a]];
    __syncthreads();
    if (A.rec_every && t < A.M.S) {
        int c = 0;
        for (int a = 0; a < n; a++) c += mc_spec[a] == t;
        count[t] = c;
    }
    __syncthreads();
    // (everything below is the same in every thread: the proposal, the decision and the counters are computed redundantly)
    double E = A.energy[f];
    long long acc_n = A.accepted[f], tri_n = A.trials[f];
    const double kT = A.kT[f];
    int n_allowed = 0;
    for (int s = 0; s < A.M.S; s++) n_allowed += A.mu[s] > -__builtin_inf();
    int status = UF3_MC_RUNNING;
    for (int k = 0; k < A.n_trials; k++) {
        const unsigned long long tt = A.t0 + (unsigned long long)k;
        const uint4 r = md_philox(make_uint4((uint32_t)f, (uint32_t)tt, (uint32_t)(tt >> 32), 0u),
                                  make_uint2((uint32_t)A.seed, (uint32_t)(A.seed >> 32)));
        McMove mv;
        mv.i = (int)(((unsigned long long)r.x * (unsigned long long)n) >> 32);
        bool null_trial;
        double dmu = 0.0;
        if (A.mode == 0) {
            mv.j = (int)(((unsigned long long)r.y * (unsigned long long)n) >> 32);
            mv.zi = mc_spec[mv.j]; mv.zj = mc_spec[mv.i];
            null_trial = mv.i == mv.j || mv.zi == mv.zj || (A.swappable && !(A.swappable[lo + mv.i] && A.swappable[lo + mv.j]));
        } else {
            const int zo = mc_spec[mv.i];
            mv.j = -1; mv.zj = 0; mv.zi = zo;
            null_trial = (A.swappable && !A.swappable[lo + mv.i]) || !(A.mu[zo] > -__builtin_inf()) || n_allowed < 2;
            if (!null_trial) {
                int pick = (int)(((unsigned long long)r.y * (unsigned long long)(n_allowed - 1)) >> 32);
                for (int s = 0; s < A.M.S; s++) {
                    if (s == zo || !(A.mu[s] > -__builtin_inf())) continue;
                    if (pick == 0) { mv.zi = s; break; }
                    pick--;
                }
                dmu = A.mu[mv.zi] - A.mu[zo];
            }
        }
        tri_n++;
        if (!null_trial) {
            const double dE = mc_delta(A.M, A.tb, mc_spec, L, lo, mv);
            const double dEp = dE - dmu;
            if (!isfinite(dE)) { status = UF3_MC_NONFINITE; tri_n--; break; }
            const bool accept = dEp <= 0.0 || (kT > 0.0 && md_uniform(r.z, r.w) < exp(-dEp / kT));
            if (accept) {
                if (t == 0) {
                    count[mc_spec[mv.i]]--; count[mv.zi]++;
                    mc_spec[mv.i] = (unsigned char)mv.zi;
                    A.z[lo + mv.i] = A.s2z[mv.zi];
                    if (mv.j >= 0) {
                        count[mc_spec[mv.j]]--; count[mv.zj]++;
                        mc_spec[mv.j] = (unsigned char)mv.zj;
                        A.z[lo + mv.j] = A.s2z[mv.zj];
                    }
                }
                E += dE;
                acc_n++;
                __syncthreads();
            }
        }
        if (A.rec_every && (A.run_done + k + 1) % A.rec_every == 0 && t == 0) {
            double *rec = A.records + ((size_t)((A.run_done + k + 1) / A.rec_every - 1) * A.n_frames + f) * (3 + A.M.S);
            rec[0] = E; rec[1] = (double)acc_n; rec[2] = (double)tri_n;
            for (int s = 0; s < A.M.S; s++) rec[3 + s] = (double)count[s];
        }
    }
    if (t == 0) { A.energy[f] = E; A.accepted[f] = acc_n; A.trials[f] = tri_n; A.status[f] = status; }
}

struct McDeltaArgs {
    McModel M;
    McTable tb;
    const long long *offsets;
    const int32_t *z;
    const int32_t *frame, *i, *j;          // [n] proposals: frame, atom within it, second atom (swap) or new species INDEX (transmute)
    int mode;
    double *dE;                            // [n]
};

__global__ void __launch_bounds__(UF3_MC_THREADS) k_mc_delta(McDeltaArgs A) {
    extern __shared__ __align__(16) unsigned char mc_spec[];
    __shared__ McLds L;
    const int q = blockIdx.x, t = threadIdx.x;
    const int f = A.frame[q];
    const long long lo = A.offsets[f];
    const int n = (int)(A.offsets[f + 1] - lo);
    for (int a = t; a < n; a += UF3_MC_THREADS) mc_spec[a] = (unsigned char)A.M.B->z2s[A.z[lo + a]];
    __syncthreads();
    McMove mv;
    mv.i = A.i[q];
    if (A.mode == 0) { mv.j = A.j[q]; mv.zi = mc_spec[mv.j]; mv.zj = mc_spec[mv.i]; }
    else { mv.j = -1; mv.zj = 0; mv.zi = A.j[q]; }
    const double dE = mc_delta(A.M, A.tb, mc_spec, L, lo, mv);
    if (t == 0) A.dE[q] = dE;
}
