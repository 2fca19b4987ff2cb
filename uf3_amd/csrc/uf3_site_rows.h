// uf3_site_rows.h -- site rows and extrapolation grades (uf3_site_rows[_dev], uf3_site_grade[_dev], uf3_md_run_grade).
// gfx950, fp64.
//
// Site row      b_i [F], the featurizer's columns: b_i . c = U_i (uf3_flux.h's site energy) for every flat coefficient vector c.
//               Column sm gets 1 (one-body); a directed pair entry adds its four B-spline values at pair_col + (interval - 3);
//               a triplet with i as the centre adds the 64 products B_l B_m B_n at lut[raw bin] -- BasisDev::lut, the table the
//               featurizer's energy row is folded by (a raw bin outside the template has no column: -1, and its coefficient
//               in an expanded model is an exact zero).  Legs by trio_swap_legs, as k_flux_site_terms: on a symmetry-1 trio
//               the supercell-index tie-break decides the COLUMN here.
// Grade         gamma_i = |W b_i|^2 with uf3_leverage's W (lower triangular, exact zeros above the diagonal).
//
//   site_row_walk   one wave, one centre: the row accumulated in LDS.  Lanes over the pair entries, then over the (j, k)
//                   pairs of the 3-body neighbours; every product goes into the row by an LDS add.  Two lanes of one
//                   instruction may meet in one column: the LDS unit serialises them in an order that is a function of
//                   the instruction's addresses alone, and no other wave touches the row, so the sums repeat bit for bit
//                   and do not depend on the batch around the frame.
//   k_site_rows     one wave per centre: walk, then the row to HBM with plain stores.
//   k_site_grade    a workgroup of four waves owns SG_TILE = 16 centres: each wave walks four of them into the tile
//                   X [16][stride] in LDS, then Z^T = W X^T goes 16 x 16 tile by tile over the fp64 matrix cores as in
//                   k_leverage (A = W, B = X^T: an X row is a column of the accumulator, the accumulator's layout from
//                   the context's probe table, the steps wholly above the diagonal never issued), each wave its own k
//                   tiles; lane sums -> LDS -> one thread per centre adds them in a fixed order.  No row reaches HBM and
//                   W is read once per 16 atoms.
//   k_site_frame_max  one workgroup per frame: largest grade and its frame-local atom, lowest index on ties, by a
//                   fixed tree.  An empty frame: 0 and -1.
// stride = 32 ceil(F / 32) + 2 doubles: even, so that a row starts 16-byte aligned and any 16-byte access the compiler forms
// from two neighbouring columns is aligned; = 2 mod 32, so that the 32 (row, j) operands of a half-wave's 8-byte read fall on 32
// distinct bank pairs (k_leverage's LV_LDW = 66 is the same choice).  The columns [F, stride) stay zero.
#pragma once
#include "uf3_flux.h"
#include "uf3_leverage.h"

#define SG_TILE 16                       // centres per workgroup of k_site_grade (one MFMA tile of rows)
#define SG_LDS_BUDGET (80 * 1024)        // bytes per workgroup: two workgroups per CU (160 KB), one walking while the other multiplies

typedef __attribute__((address_space(3))) double LdsDouble;

__host__ __device__ __forceinline__ int site_row_stride(int n_feat) { return ((n_feat + 31) / 32) * 32 + 2; }
// LDS of k_site_grade: the tile (at least the 4 x 256 lane sums that take its place at the end) | the probe table's inverse | the
// four waves' index arrays
__host__ __device__ __forceinline__ size_t site_grade_tile_doubles(int n_feat) {
    const size_t x = (size_t)SG_TILE * site_row_stride(n_feat);
    return x < 1024 ? 1024 : x;
}
__host__ __device__ __forceinline__ size_t site_grade_lds(int n_feat, int cap) {
    return 8 * site_grade_tile_doubles(n_feat) + 4 * 256 + 4 * 4 * (size_t)cap;
}

struct SiteArgs {
    FluxArgs F;               // the lists (c1 / c2 / c3, u, w, jp, flux unused)
    long long m0, m1;         // centres [m0, m1) of the batch
    int n_feat;
    double *rows;             // k_site_rows: [m1 - m0][ld]
    long long ld;
    const double *w;          // k_site_grade: [n_feat][n_feat]
    const int *frag;          //   the accumulator layout (k_mfma_probe)
    double *grade;            //   [n]
};

__device__ __forceinline__ void site_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// The row of centre m into `row` (LDS, zeroed by the caller, [>= F]); idx3: [cap] ints of LDS of this wave's own.  false: the
// centre's list was cut (flags[1] set; the host grows the capacity and runs again).
__device__ __forceinline__ bool site_row_walk(const FluxArgs &F, long long m, int lane, int *idx3, LdsDouble *row) {
    const BasisDev *B = F.B;
    const int sm = F.spec[m];
    const int n = F.cnt[m];
    if (n > F.cap) {
        if (lane == 0) F.flags[1] = 1;
        return false;
    }
    auto add = [&](int col, double v) { __hip_atomic_fetch_add(row + col, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); };
    const HessNbr *L = F.ent + (size_t)m * F.cap;
    if (lane == 0) add(sm, 1.0);
    // pair entries, and the list positions of the 3-body neighbours (list order)
    int n3 = 0;
    for (int e0 = 0; e0 < n; e0 += WAVE) {
        const bool live = e0 + lane < n;
        const int e = live ? e0 + lane : 0;
        const HessNbr en = L[e];
        const bool is3 = live && (en.flags & 2);
        const unsigned long long mask3 = __ballot(is3);
        if (is3) idx3[n3 + mbcnt(mask3)] = e;
        n3 += __popcll(mask3);
        if (live && (en.flags & 1)) {
            const int pair_idx = sm * UF3_MAX_SPECIES + en.spec;
            const LegDev leg = B->pairs[B->pair_of[pair_idx]].leg;
            KnotRec kr;
            const int i = load_interval<1>(B->recs, leg, en.r, kr);
            double v[4];
            bspline4<false>(kr, en.r, v, nullptr);
            const int col = B->pair_col[pair_idx] + (i - 3);
            for (int q = 0; q < 4; q++) add(col + q, v[q]);
        }
    }
    site_wave_sync();
    if (B->T > 0) {
        const int npair = n3 * (n3 - 1) / 2;
        for (int p0 = 0; p0 < npair; p0 += WAVE) {
            const int p = p0 + lane;
            if (p >= npair) continue;
            int a, b;
            flux_pair_of(p, a, b);
            const HessNbr ea = L[idx3[a]], eb = L[idx3[b]];
            const bool swap = trio_swap_legs(B, sm, ea, eb, false);
            const HessNbr &ej = swap ? eb : ea, &ek = swap ? ea : eb;
            const int trio = B->trio_of[(sm * UF3_MAX_SPECIES + ej.spec) * UF3_MAX_SPECIES + ek.spec];
            if (trio < 0) continue;
            const double rl = ej.r, rm = ek.r, rn = norm3_rn(ek.dx - ej.dx, ek.dy - ej.dy, ek.dz - ej.dz);
            // trio_value's support test and intervals, without the coefficients
            const TrioDev *td = B->trios + trio;
            const LegDev l0 = td->leg[0], l1 = td->leg[1], l2 = td->leg[2];
            if (!((rl > l0.t0) & (rl < l0.tlast) & (rm > l1.t0) & (rm < l1.tlast) & (rn > l2.t0) & (rn < l2.tlast))) continue;
            KnotRec kl, km, kn;
            const int il = load_interval<1>(B->recs, l0, rl, kl), im = load_interval<1>(B->recs, l1, rm, km),
                      in = load_interval<1>(B->recs, l2, rn, kn);
            double vl[4], vm[4], vn[4];
            bspline4<false>(kl, rl, vl, nullptr);
            bspline4<false>(km, rm, vm, nullptr);
            bspline4<false>(kn, rn, vn, nullptr);
            const int dim_n = td->dim_n, mn = td->dim_m * dim_n;
            const int *lut = B->lut + td->lut_off + (size_t)(il - 3) * mn + (im - 3) * dim_n + (in - 3);
            for (int x = 0; x < 4; x++)
                for (int y = 0; y < 4; y++) {
                    const double lm = vl[x] * vm[y];
                    const int *lp = lut + x * mn + y * dim_n;
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int col = lp[q];
                        if (col >= 0) add(col, lm * vn[q]);
                    }
                }
        }
    }
    site_wave_sync();
    return true;
}

// dynamic LDS: [stride] doubles (the row) | [cap] ints
__global__ void __launch_bounds__(64) k_site_rows(SiteArgs A) {
    extern __shared__ __attribute__((aligned(16))) double site_lds[];
    const long long m = A.m0 + blockIdx.x;
    const int lane = threadIdx.x;
    if (m >= A.m1) return;
    const int stride = site_row_stride(A.n_feat);
    LdsDouble *row = (LdsDouble *)site_lds;
    int *idx3 = (int *)(site_lds + stride);
    for (int j = lane; j < stride; j += WAVE) row[j] = 0.0;
    site_wave_sync();
    if (!site_row_walk(A.F, m, lane, idx3, row)) return;
    double *dst = A.rows + (size_t)(m - A.m0) * A.ld;
    for (int j = lane; j < A.n_feat; j += WAVE) dst[j] = row[j];
}

// dynamic LDS: site_grade_lds(n_feat, cap)
__global__ void __launch_bounds__(256, 2) k_site_grade(SiteArgs A) {
    extern __shared__ __attribute__((aligned(16))) double site_lds[];
    const int t = threadIdx.x, lane = t & 63;
    const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
    const int F = A.n_feat, stride = site_row_stride(F);
    const size_t xd = site_grade_tile_doubles(F);
    double *X = site_lds;
    int *inv = (int *)(site_lds + xd);                                 // [16 r][16 k] -> lane * 4 + v
    int *idx3 = inv + 256 + wave * A.F.cap;
    const long long r0 = A.m0 + (long long)blockIdx.x * SG_TILE;
    {
        const int fr = A.frag[2 * t], fc = A.frag[2 * t + 1];
        inv[fc * 16 + fr] = t;
    }
    for (int j = t; j < SG_TILE * stride; j += 256) X[j] = 0.0;
    __syncthreads();
    // rows wave, wave + 4, ...: every wave the same number of trips (a centre past the end is an empty one)
    for (int q = 0; q < SG_TILE / 4; q++) {
        const int r = wave + 4 * q;
        if (r0 + r < A.m1) site_row_walk(A.F, r0 + r, lane, idx3, (LdsDouble *)(X + (size_t)r * stride));
    }
    __syncthreads();
    // operand roles of the lane: A = W[16 kt + (lane & 15)][j0 + (lane >> 4)], B = X[lane & 15][j0 + (lane >> 4)]
    const int li = lane & 15, lk = lane >> 4;
    const double *xb = X + li * stride + lk;
    int fk[4];
#pragma unroll
    for (int v = 0; v < 4; v++) fk[v] = A.frag[(lane * 4 + v) * 2];
    double sq[4] = {0.0, 0.0, 0.0, 0.0};
    const int nt = (F + 15) >> 4;
    for (int kt = wave; kt < nt; kt += 4) {
        const int k = kt * 16 + li;
        const double *wrow = A.w + (size_t)(k < F ? k : 0) * F;
        double4_t acc = double4_t{0, 0, 0, 0};
        const int np = kt + 1;                                          // pieces of 16 j: j0 < 16 kt + 16, the last the diagonal piece
        double a[4];
        auto load_w = [&](int pc) {
#pragma unroll
            for (int e = 0; e < 4; e++) {
                const int j = pc * 16 + 4 * e + lk;
                a[e] = wrow[j < F ? j : 0];                            // (j >= F meets the tile's zero columns, k >= F is dropped below)
            }
        };
        load_w(0);
        for (int pc = 0; pc < np; pc++) {
            const double ac[4] = {a[0], a[1], a[2], a[3]};
            load_w(pc + 1 < np ? pc + 1 : pc);
#pragma unroll
            for (int e = 0; e < 4; e++) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(ac[e], xb[pc * 16 + 4 * e], acc, 0, 0, 0);
        }
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const double z = kt * 16 + fk[v] < F ? acc[v] : 0.0;
            sq[v] += z * z;
        }
    }
    // the lanes' sums take the tile's place: part[wave][lane * 4 + v]; thread r adds the 4 x 16 values of row r, waves then k
    __syncthreads();
#pragma unroll
    for (int v = 0; v < 4; v++) X[wave * 256 + lane * 4 + v] = sq[v];
    __syncthreads();
    if (t < SG_TILE && r0 + t < A.m1) {
        double rs = 0.0;
        for (int wq = 0; wq < 4; wq++)
            for (int k = 0; k < 16; k++) rs += X[wq * 256 + inv[t * 16 + k]];
        A.grade[r0 + t] = rs;
    }
}

// offsets: the caller's [n_frames + 1] (empty frames allowed).  fmax / fargmax: [n_frames] each, either may be null; pair:
// [n_frames][2] = (max, argmax as a double) or null.
__global__ void __launch_bounds__(256) k_site_frame_max(const double *grade, const int64_t *offsets, double *fmax, int32_t *fargmax,
                                                        double *pair) {
    __shared__ double sv[256];
    __shared__ long long si[256];
    const int f = blockIdx.x, t = threadIdx.x;
    const long long lo = offsets[f], hi = offsets[f + 1];
    double bv = 0.0;
    long long bi = -1;
    for (long long i = lo + t; i < hi; i += 256) {
        const double g = grade[i];
        if (bi < 0 || g > bv) { bv = g; bi = i - lo; }      // (ascending i: the first of equal values stays)
    }
    sv[t] = bv; si[t] = bi;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) {
            const double ov = sv[t + s];
            const long long oi = si[t + s];
            if (oi >= 0 && (si[t] < 0 || ov > sv[t] || (ov == sv[t] && oi < si[t]))) { sv[t] = ov; si[t] = oi; }
        }
        __syncthreads();
    }
    if (t == 0) {
        if (fmax) fmax[f] = sv[0];
        if (fargmax) fargmax[f] = (int32_t)si[0];
        if (pair) { pair[2 * (size_t)f] = sv[0]; pair[2 * (size_t)f + 1] = (double)si[0]; }
    }
}
