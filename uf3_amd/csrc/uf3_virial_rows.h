// uf3_virial_rows.h -- the strain derivative of the energy row: six more rows of the design matrix per frame.
//
//   k_virial_rows<MODE>   x_v [n_frames][6][F] (fp64), Voigt order xx, yy, zz, yz, xz, xy, the convention of uf3_eval_virial:
//                         x_v[f][q][:] = d x_e[f][:] / d t for the strain eps_aa = t (q < 3) or eps_ab = eps_ba = t / 2 (q >= 3),
//                         applied to cell and positions alike, so that x_v[f] @ c is what the evaluator returns for coefficients c
//                         MODE 0      pair columns, from the featurizer's cell list and candidate walk
//                         MODE 1-5    3-body columns, from the lists the MODE 0 launch of k_featurize (or k_build_n3) left in
//                                     N3Lists; (sources per column, 64-column chunks per walk) = (1,1) (1,2) (2,1) (2,2) (6,1)
//
// The model is linear in its coefficients, so the rows are the energy row's sums with every term B(r) replaced by its strain
// derivative: a bond d of length r changes by d r / d t = d_a d_b / r under either strain above, hence
//     pair     B'(r) d_a d_b / r                                       for every directed bond the energy row counts
//     triplet  sum over the legs l, m, n of  (d/d r_leg of B_l B_m B_n) d^leg_a d^leg_b / r_leg
// with every triplet taken once, at its centre, exactly the triplets (and weights) of the energy row: the walk is the energy-only
// walk of trio_block (trio_walk_setup / trio_walk_geom with the neighbour role switched off).  The bond vectors are the image
// vectors the walk and the lists hold -- never positions -- so the rows do not change when single atoms move by lattice vectors.
// One-body columns stay zero, and so does every column the energy row leaves at zero (the frozen columns have no entry in
// colsrc and lie outside [lead2, nb - trail2)).
//
// Structure: that of the energy-only instances of k_featurize.  One wave per atom, lanes own columns, the walk gathers into six
// sums a lane (registers), ONE add per (atom, column, component) into the block-shared LDS row set [6][FE], which is flushed to
// HBM with atomics at every frame change inside the workgroup and at its end, as erow is.  Per-triplet LDS atomics of a wave
// onto the few columns of a shell serialise: the pair launch therefore adds into a per-wave row buffer
// first, as pair_rows does.  Where the six rows do not fit (v_direct, decided by the host from this carve) the adds go straight
// to HBM.  Atoms far outside their cell are refused by the host: the image-range rule of the reference's force rows has no
// strain analogue.
#pragma once
#include "uf3_kernels.h"

#define VSTAGE 16         // triplet records staged in LDS per wave at a time
#define VREC_STRIDE 46    // doubles per staged record (16-B aligned):
// 0-7 (Bl,B'l)[4], 8-15 (Bm,B'm)[4], 16-23 (Bn,B'n)[4], 24-29 Wl[6], 30-35 Wm[6], 36-41 Wn[6] (W = d_a d_b / r of the leg),
// 42-43 int4 {first l, first m, first n, -}, 44-45 zero pair

// where a wave adds its six sums of a column: the block's LDS row set, or (atoms of a frame other than the one the LDS rows
// currently hold, or rows too long for LDS) straight to HBM
struct VSink {
    double *lds;     // [6][fe_pad], column 0 = global column col_lo
    double *glob;    // x_v block of this atom's frame [6][F]
    int fe_pad, col_lo, F;
    bool direct;
    __device__ __forceinline__ void add(int q, int col, double v) const {
        if (v == 0.0) return;
        if (direct) unsafeAtomicAdd(glob + (size_t)q * F + col, v); else lds_add(lds + (size_t)q * fe_pad + (col - col_lo), v);
    }
};

__device__ __forceinline__ void voigt_weights(double dx, double dy, double dz, double r, double *w) {
    const double ir = 1.0 / r;
    w[0] = dx * dx * ir; w[1] = dy * dy * ir; w[2] = dz * dz * ir;
    w[3] = dy * dz * ir; w[4] = dx * dz * ir; w[5] = dx * dy * ir;
}

template <int NSRC, int NCH>
__device__ __forceinline__ void virial_gather_one(const double *rec, const ColSrc (&src)[NCH][NSRC], double (&acc)[NCH][6]) {
    const int4 mt = *(const int4 *)(rec + 42);
    double wl[6], wm[6], wn[6];
#pragma unroll
    for (int q = 0; q < 6; q += 2) {
        const double2 a = *(const double2 *)(rec + 24 + q), b = *(const double2 *)(rec + 30 + q), c = *(const double2 *)(rec + 36 + q);
        wl[q] = a.x; wl[q + 1] = a.y; wm[q] = b.x; wm[q + 1] = b.y; wn[q] = c.x; wn[q + 1] = c.y;
    }
#pragma unroll
    for (int ch = 0; ch < NCH; ch++) {
#pragma unroll
        for (int k = 0; k < NSRC; k++) {
            const unsigned a = (unsigned)(src[ch][k].l - mt.x), b = (unsigned)(src[ch][k].m - mt.y),
                           c = (unsigned)(src[ch][k].n - mt.z);
            const bool ok = (a | b | c) < 4u;
            const double2 L = *(const double2 *)(rec + 2 * (a & 3u));
            const double2 M = *(const double2 *)(rec + 8 + 2 * (b & 3u));
            // out-of-block sources read the record's zero pair: all three products vanish
            const double2 N = *(const double2 *)(rec + (ok ? 16 + 2 * (c & 3u) : 44));
            const double p1 = L.y * (M.x * N.x), p2 = M.y * (L.x * N.x), p3 = N.y * (L.x * M.x);
#pragma unroll
            for (int q = 0; q < 6; q++) acc[ch][q] = fma(p3, wn[q], fma(p2, wm[q], fma(p1, wl[q], acc[ch][q])));
        }
    }
}

// 64 evaluated triplets (one per lane) pass through the wave's VSTAGE-record LDS stage in quarters
template <int NSRC, int NCH>
__device__ __forceinline__ void virial_stage_and_gather(const TripletRec &r, const double (&wt)[3][6], bool valid, double *stage,
                                                        const ColSrc (&src)[NCH][NSRC], double (&acc)[NCH][6]) {
    const int lane = lane_id();
    for (int part = 0; part < WAVE / VSTAGE; part++) {
        const bool mine = valid && ((lane / VSTAGE) == part);
        const unsigned long long mask = __ballot(mine);
        if (mask == 0) continue;
        if (mine) {
            double *rec = stage + (size_t)mbcnt(mask) * VREC_STRIDE;
            for (int leg = 0; leg < 3; leg++) {
                for (int q = 0; q < 4; q++) { rec[8 * leg + 2 * q] = r.v[leg][q]; rec[8 * leg + 2 * q + 1] = r.d[leg][q]; }
                for (int q = 0; q < 6; q++) rec[24 + 6 * leg + q] = wt[leg][q];
            }
            *(int4 *)(rec + 42) = make_int4(r.first[0], r.first[1], r.first[2], 0);
            rec[44] = 0.0; rec[45] = 0.0;
        }
        wave_sync();
        const int n_staged = __popcll(mask);
        for (int q = 0; q < n_staged; q++) virial_gather_one<NSRC, NCH>(stage + (size_t)q * VREC_STRIDE, src, acc);
        wave_sync();
    }
}

// the 3-body columns of trio block t that atom m centres
template <int NSRC, int NCH>
__device__ __forceinline__ void virial_trio_block(const FeatArgs &A, const FrameGeom &g, const WaveLds &w, int m, int sm, int t,
                                                  const VSink &vs) {
    const int lane = lane_id();
    const TrioDev td_copy = load_const(A.trios + t);
    const TrioDev *td = &td_copy;
    TrioWalk k;
    trio_walk_setup<false, false>(A, w, td->sc, td->sa, td->sb, sm, k);       // centre role only
    if (k.n_items == 0) return;
    const int ncol = td->ncol;
    for (int c0 = 0; c0 < ncol; c0 += NCH * WAVE) {
        ColSrc src[NCH][NSRC];
        double acc[NCH][6];
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) for (int u = 0; u < 6; u++) acc[ch][u] = 0.0;
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) {
            const int col = c0 + ch * WAVE + lane;
#pragma unroll
            for (int q = 0; q < NSRC; q++) {
                const int sp = col < ncol ? A.colsrc[td->src_off + col * NSRC + q] : -1;
                src[ch][q].l = sp < 0 ? (1 << 20) : (sp & 255);
                src[ch][q].m = (sp >> 8) & 255;
                src[ch][q].n = (sp >> 16) & 255;
            }
        }
        for (int p0 = 0; p0 < k.n_items; p0 += WAVE) {
            TripletGeom tg;
            TripletRec r;
            bool valid = trio_walk_geom<false, false>(A, g, w, td->sa, td->sb, k, m, sm, p0 + lane, tg);
            valid = eval_triplet<true>(A.recs, td, tg, valid, r);
            double wt[3][6];
            if (valid) {
                // the legs' own image vectors, from the list: centre -> a, centre -> b, a -> b
                const double ax = w.ox[tg.i1], ay = w.oy[tg.i1], az = w.oz[tg.i1];
                const double bx = w.ox[tg.i2], by = w.oy[tg.i2], bz = w.oz[tg.i2];
                voigt_weights(ax, ay, az, tg.rl, wt[0]);
                voigt_weights(bx, by, bz, tg.rm, wt[1]);
                voigt_weights(bx - ax, by - ay, bz - az, tg.rn, wt[2]);
            }
            virial_stage_and_gather<NSRC, NCH>(r, wt, valid, w.stage, src, acc);
        }
#pragma unroll
        for (int ch = 0; ch < NCH; ch++) {
            const int col = c0 + ch * WAVE + lane;
            if (col < ncol)
#pragma unroll
                for (int q = 0; q < 6; q++) vs.add(q, td->col + col, acc[ch][q]);
        }
    }
}

// the pair columns of atom m: lanes <-> neighbour images as the candidate walk hands them out.  Each lane evaluates its bond
// and adds B' d_a d_b / r into the wave's row buffer [6][n2] (bonds of one shell hit the same four columns); the buffer then
// goes to the block's rows, one add per column and component.
__device__ __forceinline__ void virial_pair_rows(const FeatArgs &A, const BasisDev *B, const FrameGeom &g, double *row, int m, int sm,
                                                 const double *pm, const VSink &vs) {
    const int lane = lane_id(), S = load_const(&B->S);
    const int n2 = A.n_pair_cols;
    const int pairs_uniform = load_const(&B->pairs_uniform), lead2 = load_const(&B->lead2), trail2 = load_const(&B->trail2);
    for (int q = lane; q < 6 * n2; q += WAVE) row[q] = 0.0;
    wave_sync();
    for_each_candidate(g, A.cl, m, [&](bool ok, const SlotRec &sr, int sj, int s0, int s1, int s2) {
        if (!ok) return;
        double dx, dy, dz;
        image_delta(g, sr, s0, s1, s2, pm, dx, dy, dz);
        const double d = norm3_rn(dx, dy, dz);
        const int pair_idx = sm * UF3_MAX_SPECIES + sj;
        const PairDev &pd = B->pairs[pairs_uniform ? 0 : B->pair_of[pair_idx]];
        const double p_rmin = pd.rmin, p_rmax = pd.rmax;
        if (!(d > p_rmin && d < p_rmax)) return;                   // distances.py:66, strict both sides
        const LegDev leg = pd.leg;
        const int p_nb = pd.nb, p_col = B->pair_col[pair_idx];
        KnotRec kr;
        double v[4], dv[4], wt[6];
        const int first = load_interval<1>(A.recs, leg, d, kr) - 3;
        bspline4<true>(kr, d, v, dv);
        voigt_weights(dx, dy, dz, d, wt);
        const int hi = p_nb - trail2, base = p_col - S;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int bf = first + q;
            if (bf >= lead2 && bf < hi) {                          // bspline.py:840,880
                double *dst = row + base + bf;
#pragma unroll
                for (int u = 0; u < 6; u++) lds_add(dst + u * n2, dv[q] * wt[u]);
            }
        }
    });
    wave_sync();
    for (int col = lane; col < n2; col += WAVE)
#pragma unroll
        for (int u = 0; u < 6; u++) vs.add(u, S + col, row[u * n2 + col]);
    wave_sync();
}

// LDS carve (must match virial_lds_bytes on the host): the row set [6][fe_pad] (absent when v_direct), then per wave
// MODE 0: the row buffer [6][n2];  MODE 1-5: the own list ox | oy | oz | orr [cap] and the stage, then the species offsets (ints)
template <int MODE>
__global__ void __launch_bounds__(WPB * WAVE, 2)
k_virial_rows(FeatArgs A, double *x_v, int v_direct) {
    extern __shared__ __align__(16) unsigned char smem[];
    const BasisDev *B = A.B;
    const int F = load_const(&B->F), S = load_const(&B->S), n_trios = load_const(&B->T), cap = A.n3.cap;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    double *vrow = (double *)smem;
    const bool v_lds = !v_direct;
    // (the pair launch adds to the pair columns only, a trio launch to the 3-body columns only: the rows hold just those)
    const int col_lo = MODE == 0 ? S : S + A.n_pair_cols;
    const int FE = MODE == 0 ? A.n_pair_cols : F - col_lo;
    const int fe_pad = FE + (FE & 1);
    const size_t v_d = v_lds ? 6 * (size_t)fe_pad : 0;
    const size_t list_d = MODE == 0 ? 0 : 4 * (size_t)cap;
    const size_t stage_d = MODE == 0 ? 6 * (size_t)A.n_pair_cols : (size_t)VSTAGE * VREC_STRIDE;
    const size_t per_wave_d = list_d + stage_d + ((list_d + stage_d) & 1);
    const size_t per_wave_i = MODE == 0 ? 0 : UF3_MAX_SPECIES + 2;
    double *wd = vrow + v_d + (size_t)wave * per_wave_d;
    int *wi = (int *)(vrow + v_d + (size_t)WPB * per_wave_d) + (size_t)wave * per_wave_i;
    WaveLds w;
    w.ox = wd; w.oy = w.ox + cap; w.oz = w.oy + cap; w.orr = w.oz + cap; w.oir = nullptr;
    w.stage = wd + list_d;
    w.oparent = nullptr; w.oshift = nullptr; w.osidx = nullptr; w.noff = nullptr; w.nbase = nullptr; w.ospoff = nullptr;
    w.so = wi;
    w.sp_stride = S + 1;
    w.geo = nullptr; w.cand = nullptr; w.pstage = nullptr;

    if (v_lds) for (int q = tid; q < 6 * fe_pad; q += WPB * WAVE) vrow[q] = 0.0;
    __syncthreads();
    // (atoms to workgroups as in k_featurize: every XCD one contiguous eighth of the atoms)
    const int bid = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int block_first = bid * A.atoms_per_block;
    const int block_end = min(block_first + A.atoms_per_block, A.natoms);
    int vrow_frame = -1;
    FrameGeom g;
    int g_frame = -1;
    for (int m0 = block_first; m0 < block_end; m0 += WPB) {
        const int m = m0 + wave;
        const bool active = m < block_end;
        if (v_lds) {
            const int f_first = load_const(A.frame_of + m0);
            if (f_first != vrow_frame) {                          // block-uniform
                __syncthreads();
                if (vrow_frame >= 0)
                    for (int q = tid; q < 6 * fe_pad; q += WPB * WAVE) {
                        const double v = vrow[q];
                        const int u = q / fe_pad, col = q - u * fe_pad;
                        if (v != 0.0 && col < FE) { unsafeAtomicAdd(x_v + ((size_t)vrow_frame * 6 + u) * F + col_lo + col, v); vrow[q] = 0.0; }
                    }
                __syncthreads();
                vrow_frame = f_first;
            }
        }
        if (!active) continue;
        const int fr = load_const(A.frame_of + m);
        if (fr != g_frame) { g = A.geoms[fr]; g_frame = fr; }
        const int sm = ((const __attribute__((address_space(4))) signed char *)(unsigned long long)A.spec)[m];
        VSink vs;
        vs.lds = vrow; vs.glob = x_v + (size_t)fr * 6 * F; vs.fe_pad = fe_pad; vs.col_lo = col_lo; vs.F = F;
        vs.direct = !v_lds || (fr != vrow_frame);
        if (MODE == 0) {
            const double pm[3] = {A.pos[3 * (size_t)m], A.pos[3 * (size_t)m + 1], A.pos[3 * (size_t)m + 2]};
            virial_pair_rows(A, B, g, w.stage, m, sm, pm, vs);
        } else if (n_trios > 0) {
            const int n = min(load_const(A.n3.cnt + m), cap);
            const size_t base = (size_t)m * cap;
            wave_sync();
            for (int e = lane; e < n; e += WAVE) {
                const N3Entry en = A.n3.ent[base + e];
                w.ox[e] = en.dx; w.oy[e] = en.dy; w.oz[e] = en.dz; w.orr[e] = en.r;
            }
            if (lane <= S) w.so[lane] = min(A.n3.spoff[(size_t)m * (UF3_MAX_SPECIES + 1) + lane], n);
            wave_sync();
            for (int t = 0; t < n_trios; t++) {
                const TrioDev *td = A.trios + t;
                typedef int int8_v __attribute__((ext_vector_type(8)));
                const int8_v hv = *(const __attribute__((address_space(4))) int8_v *)(unsigned long long)&td->head;
                const TrioHead th = {hv[0], hv[1], hv[2], hv[3], hv[4], hv[5], hv[6], hv[7]};
                // (by sources and width alone: the matrix-core windows of the force rows play no part here)
                const int t_mode = th.nsrc == 1 ? (th.ncol > WAVE ? 2 : 1) : (th.nsrc == 2 ? (th.ncol > WAVE ? 4 : 3) : 5);
                if (t_mode != MODE || th.sc != sm) continue;
                if (MODE == 1) virial_trio_block<1, 1>(A, g, w, m, sm, t, vs);
                else if (MODE == 2) virial_trio_block<1, 2>(A, g, w, m, sm, t, vs);
                else if (MODE == 3) virial_trio_block<2, 1>(A, g, w, m, sm, t, vs);
                else if (MODE == 4) virial_trio_block<2, 2>(A, g, w, m, sm, t, vs);
                else virial_trio_block<6, 1>(A, g, w, m, sm, t, vs);
            }
        }
    }
    if (v_lds) {
        __syncthreads();
        if (vrow_frame >= 0)
            for (int q = tid; q < 6 * fe_pad; q += WPB * WAVE) {
                const double v = vrow[q];
                const int u = q / fe_pad, col = q - u * fe_pad;
                if (v != 0.0 && col < FE) unsafeAtomicAdd(x_v + ((size_t)vrow_frame * 6 + u) * F + col_lo + col, v);
            }
    }
}
