// uf3_feat3.h -- 3-body force (and energy) rows by BOND FACTORISATION: k_featurize3 (round 4).  gfx950 only.
//
// Reference: uf3/representation/angles.py:142-286 (featurize_force_3b / arrange_deriv_3b), :17-139 (energy), :424-632
// (triplets, leg values and derivatives).  Same gather formulation as k_featurize's trio blocks (an atom m collects the
// triplets it centres and those in which it is a neighbour of a centre e), but the sum over the triplets is taken in two
// stages instead of one rank-2 update of the (component, l) x (m, n) window per triplet:
//
//   every term of m's rows has the form   T_f[c][i] * ( sum over the triplets that share the bond f )  P_g[j] Q[n]
//   where f is a bond of m that stays fixed -- (m, a) when m is the centre and a sits on one centre leg, (m, e) when m is a
//   neighbour of the centre e -- and g is the bond on the OTHER centre leg ((m, b), or (e, k)), Q the values of leg n:
//
//   stage 1 (per triplet, 4 multiply-adds per lane):   W_s[j][n] += P_s[j] Q_s[n]          s = x, y, z, plain
//       centre role     P = (u_g,x B'(r_g), u_g,y B'(r_g), u_g,z B'(r_g), B(r_g))[j]     Q = B_n(r_ab)[n]
//       neighbour role  P = B(r_ek)[j]     Q = (a3_x B_n'(r_mk), a3_y B_n', a3_z B_n', B_n(r_mk))[n]      a3 = unit(m -> k)
//   stage 2 (per BOND f, 7 multiply-adds per window row and lane):
//       X_c[i][j][n] += T_f[i][c] W_plain[j][n] + T_f[i][plain] W_c[j][n],     X_e[i][j][n] += T_f[i][plain] W_plain[j][n]
//       T_f[i] = (u_f,x B'(r_f)[i], u_f,y B'(r_f)[i], u_f,z B'(r_f)[i], B(r_f)[i]),  u_f = unit(m -> other end of f)
//
// An atom of the benchmark has 273 triplet records but only ~50 (bond, block) pairs: the expansion over the three force
// components and the window of the fixed leg -- what the matrix cores did per record -- happens once per bond.  Lanes are the
// (j, n) positions of the W window (27 for the default trims) twice over: lanes 0-31 keep the sums (x, y) of a position, lanes
// 32-63 (z, plain).  No matrix cores, no per-record staging of three evaluated legs: a record is the n-leg values (centre
// role) or those, their derivatives times a3 and the values of bond (e, k).  DESIGN.md section 3.6.
//
// Orientation: the fixed bond sits on leg l ("normal": rows i = l, window j = m) or on leg m ("transposed": i = m, j = l); a
// block has one orientation per atom species -- transposed exactly when sa != sb and the atom is of species sb (then it is
// always the SECOND neighbour, and its centre-role triplets are summed with the bond on leg m fixed instead).  Blocks with
// sa == sb must fold symmetrically in (l, m) -- column(l, m, n) = raw(l, m, n) + raw(m, l, n) -- so that which of two equal
// neighbours is "first" (angles.py:456-470, incl. the ghost-centre numbering quirk) does not matter; uf3_basis_create checks
// that and everything else this kernel assumes (Feat3 eligibility) and the other launches remain for the rest.
#pragma once

struct Feat3Leg {
    double t0, tlast, inv_h;
    int nk, row0;              // knots; number of the leg's first window row (one per knot interval from 3 on)
};

struct Feat3Args {
    const BasisDev *B;
    const TrioDev *trios;
    const double *rows;        // window rows [n_rows][18]: t_i, t_i+1 | 4 functions x (c0 c1 c2 c3), see uf3_basis_create
    int n_rows;
    const unsigned short *fsrc; // fold tables: per trio [orientation 0 | 1][column][source 0 | 1] -> index of the source bin in the fold's
                               // dump (row f of the fixed leg, position of (j, n): uf3_basis_create), or of a zero
    const int *trio_fsrc;      // [T] first entry of a trio's table
    int n_fsrc;
    Feat3Leg leg_p, leg_n;     // the centre legs (l and m share knots and window), leg n
    int lo_p, ext_p, lo_n, ext_n;
    int pr_rows;               // window rows (of the summed leg) per round of 32 positions: 32 / ext_n, at most ext_p
    const FrameGeom *geoms;
    const int *frame_of;
    N3Lists n3;
    const double *pos;
    const signed char *spec;
    double *x_e, *x_f;
    int ld;                    // doubles between consecutive force rows (>= F)
    int natoms, atoms_per_block, e_direct;
    const int *sel;            // instance selection on the device (uf3_featurize_dev launches two instances back to back when the
    int sel_mode, sel_cap;     // context's list capacity is above 16): 0 always run; 1 run iff *sel <= sel_cap; 2 iff *sel > sel_cap
    int skip;                  // ablations (-DUF3_ABLATE builds only): 1 stage 1, 2 stage 2, 4 centre walk, 8 neighbour walk, 16 fold + stores, 32 bond tables, 64 leg evaluations of the walks
};

// Compile-time shape of a launch: EF = rows of the window on the fixed leg (= ext of the centre legs), NR = rounds of 32 W
// positions per half-wave (ext_p * ext_n <= 32 NR - 1: one position stays free as the fold's zero), the strides that follow.
template <int EF, int NR>
struct F3Cfg {
    static constexpr int PS = 32 * NR;                           // positions per fixed-leg row in the fold's dump
    static constexpr int EFP = (EF + 1) & ~1;                    // dense bond values of a neighbour-role record, padded
    static constexpr int RS_N = EFP + 16 + (NR == 1 ? 2 : 0);    // doubles per neighbour-role record: B(r_ek)[ext_p] | (a3 B_n', B_n) x 4 (| pad: 44 dwords apart, the
                                                                 // eight lanes of a 16-byte store group hit different banks -- and the quad of zeros, kept
                                                                 // zero, that stage 1 reads for an n slot outside the record's four functions.  The wide
                                                                 // windows have no LDS to spare for a pad: they select the address of `zq` instead)
    static constexpr int RS_C = NR == 1 ? 10 : (NR == 2 ? 12 : 14);   // ... per centre-role record: B_n over the n window (ext_n < RS_C), zero-padded
    static constexpr int NREC = NR == 1 ? 29 : 32;               // neighbour-role records per engine pass
    static constexpr int DUMP = NR == 1 ? 4 * EF * 32 : 2 * (EF * PS + 2);   // the fold's dump: pairs of all four rows | one component per half at a time
    static constexpr int STAGE0 = 64 * RS_C > NREC * RS_N ? 64 * RS_C : NREC * RS_N;
    static constexpr int STAGE = (STAGE0 > DUMP ? STAGE0 : DUMP) + 4;  // + a quad of zeros
    static constexpr int MIN_WAVES = NR == 1 ? 4 : 2;            // waves per SIMD the registers are bounded for
};

typedef double __attribute__((ext_vector_type(2))) F3Pair;
typedef const __attribute__((address_space(3))) F3Pair *F3LdsPairs;
typedef const __attribute__((address_space(3))) double *F3LdsDoubles;
// an 8-byte LDS read the compiler may not merge with its neighbour: two reads off one base register become ONE two-address
// ds_read2_b64, which takes 8.3 cycles of the CU's LDS where two ds_read_b64 take 4.9 (tools/experiments/lds_read_bench.hip,
// DESIGN.md section 3.6).  The read stays the compiler's own -- it places and counts the waits -- and nothing else about it is
// volatile: the memory it reads is written before the wave_sync in front of it.
typedef const volatile __attribute__((address_space(3))) double *F3LdsSingles;
// entry i of a per-wave list array, read singly where the instance says so (LIST1 in the kernel) and as the plain expression
// otherwise: behind a function the wide instances allocate differently and spill two more scalar registers
#define F3_LIST(a, i) (LIST1 ? *(F3LdsSingles)((a) + (i)) : (a)[i])
// the LDS byte address of p as a scalar the compiler takes as it is: a stage-1 trip adds its per-lane offset to it in ONE vector
// instruction and advances it on the scalar unit (left to itself the compiler splits the constant part of the address off into a
// vector add of its own, or keeps vector induction variables per pointer)
__device__ __forceinline__ unsigned f3_lds_addr(const double *p) { return (unsigned)(size_t)(F3LdsDoubles)p; }
__device__ __forceinline__ unsigned f3_lds_base(unsigned a) {
    a = __builtin_amdgcn_readfirstlane(a);
    asm("" : "+s"(a));
    return a;
}

// four consecutive window functions of a leg at x (t0 < x < tlast): values v, derivatives d; returns the knot interval.
// The row of the guessed interval is fetched whole and again only when the guess was off (non-uniform knots, x on a knot).
#ifndef F3_ROWS_GLOBAL
#define F3_ROWS_GLOBAL 0
#endif
typedef const __attribute__((address_space(1))) F3Pair *F3GlobalPairs;
// (NF: how many of the four the caller uses, from the first on -- the rest of the row is not fetched and v, d keep what they held)
template <bool DERIV, int NF = 4>
__device__ __forceinline__ int f3_eval(const double *rows, const Feat3Leg &lg, double x, double (&v)[4], double (&d)[4]) {
    const int hi = lg.nk - 5;
    int iv = 3 + (int)((x - lg.t0) * lg.inv_h);
    iv = iv < 3 ? 3 : (iv > hi ? hi : iv);
    F3Pair kn, cf[2 * NF];
    auto load_row = [&](int i) {
#if F3_ROWS_GLOBAL
        F3GlobalPairs q = (F3GlobalPairs)(const F3Pair *)(rows + (size_t)(lg.row0 + i - 3) * 18);
#else
        F3LdsPairs q = (F3LdsPairs)(const F3Pair *)(rows + (size_t)(lg.row0 + i - 3) * 18);
#endif
        F3Pair t0 = q[0], t[2 * NF];
#pragma unroll
        for (int e = 0; e < 2 * NF; e++) t[e] = q[1 + e];
        kn = t0;
#pragma unroll
        for (int e = 0; e < 2 * NF; e++) cf[e] = t[e];
        __builtin_amdgcn_sched_group_barrier(F3_ROWS_GLOBAL ? 0x020 : 0x100, 1 + 2 * NF, 0);
    };
    load_row(iv);
    if (__builtin_expect(x > kn.y && iv < hi, 0)) {
        do { ++iv; load_row(iv); } while (x > kn.y && iv < hi);
    } else if (__builtin_expect(x <= kn.x && iv > 3, 0)) {
        do { --iv; load_row(iv); } while (x <= kn.x && iv > 3);
    }
    const double u = x - kn.x;
#pragma unroll
    for (int fq = 0; fq < NF; fq++) {
        const double c0 = cf[2 * fq].x, c1 = cf[2 * fq].y, c2 = cf[2 * fq + 1].x, c3 = cf[2 * fq + 1].y;
        double pv = fma(c3, u, c2), pd = fma(c3, u, pv);
        pv = fma(pv, u, c1); pd = fma(pd, u, pv);
        pv = fma(pv, u, c0);
        v[fq] = pv;
        if (DERIV) d[fq] = pd;
    }
    return iv;
}

// (CAP: the list capacity as a compile-time constant -- 16, what a tuned context settles on for bcc / fcc cells -- or 0 for
// the launch's run-time value: with it every per-wave LDS array sits at a constant offset from two bases, offsets that go into
// the LDS instructions' immediate fields instead of scalar registers the kernel has too few of)
#ifndef F3_CHAIN
#define F3_CHAIN 15        // which of the four shortenings of the atom's load chain are on (in the kernel; all, but for A/B builds)
#endif
#ifndef F3_WIDE_MINW
#define F3_WIDE_MINW 2     // waves per SIMD the wide-window instances (NR > 1) are bounded for
#endif
template <bool WANT_E, int EF, int NR, int CAP = 0>
__global__ void __launch_bounds__(WPB * WAVE, (NR == 1 ? 4 : F3_WIDE_MINW))
k_featurize3(Feat3Args A) {
    typedef F3Cfg<EF, NR> Cfg;
    constexpr int RS_C = Cfg::RS_C, RS_N = Cfg::RS_N, NREC = Cfg::NREC, PS = Cfg::PS, EFP = Cfg::EFP;
    // functions of a centre-leg evaluation that anything reads: a three-row window has no place for the fourth (the T table
    // stops at EF rows, stage 1 reads a record's bond values at p_lane < EF)
    constexpr int NFP = EF == 3 ? 3 : 4;
    // Which 8-byte reads are kept single (F3LdsSingles): the trips' and the flush's at one and three rounds -- the two-round
    // instances keep the compiler's pairs, their generic-capacity ones spill two to five more scalar registers with any of the
    // three read singly; the list entries of the walks and the T-table prologue at one round only (at two and three rounds they
    // cost two scalar spills each in two instances).  DESIGN.md section 3.6.
    constexpr bool TRIP1 = NR != 2, LIST1 = NR == 1;
    typedef std::conditional_t<TRIP1, F3LdsSingles, F3LdsDoubles> F3TripReads;
    // The atom's chain of dependent loads, shortened (F3_CHAIN, bit by bit): 1 the walk's gathered entry comes whole, parent and
    // shift in one load; 2 the atom's scalars in one group and its own entries, row and species byte in another, neither waiting
    // for the count; 4 a neighbour's row of species offsets asked for at once; 8 a block's fold table with its head.
    // (2 stays off in the two-round instances without the energy row: there it costs four to five vector registers, and the
    // generic one a wave per SIMD.  DESIGN.md section 3.6.)
    constexpr bool CH_KE = F3_CHAIN & 1, CH_OWN = (F3_CHAIN & 2) && (WANT_E || NR != 2), CH_ROWS = F3_CHAIN & 4, CH_FSRC = F3_CHAIN & 8;
    extern __shared__ __align__(16) unsigned char smem[];
    const BasisDev *B = A.B;
    // (cap: what the LDS arrays are laid out for -- the longest list this instance serves; ent_stride: entries per atom in the
    // batch's list array, the context's capacity)
    const int F = load_const(&B->F), S = load_const(&B->S), n_trios = load_const(&B->T), cap = CAP > 0 ? CAP : A.n3.cap;
    const int ent_stride = A.n3.cap;
    if (A.sel_mode) {
        const int seen = load_const(A.sel);                       // the batch's longest 3-body list (the list build behind us)
        if ((seen <= A.sel_cap) != (A.sel_mode == 1)) return;
    }
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // ---- LDS carve (feat3_lds_bytes on the host) ----------------------------------------------------------------------
    double *erow = (double *)smem;
    const bool e_lds = WANT_E && !A.e_direct;
    const size_t e_d = e_lds ? (size_t)F + (F & 1) : 0;
    double *rows_lds = erow + e_d;                                    // window rows, shared
    const double *rows = F3_ROWS_GLOBAL ? A.rows : rows_lds;
    const size_t rows_d = (size_t)A.n_rows * 18;
    const size_t list_d = 5 * (size_t)cap + ((5 * cap) & 1), tq_d = (size_t)cap * EF * 4;
    constexpr size_t stage_d = Cfg::STAGE;
    const size_t per_wave_d = list_d + tq_d + stage_d;
    const size_t per_wave_i = 2 * (size_t)cap + 2 * ((size_t)cap + 1) + (UF3_MAX_SPECIES + 2) + (size_t)cap * (S + 1) + cap;
    double *wd = rows_lds + rows_d + (size_t)wave * per_wave_d;
    int *wi = (int *)(rows_lds + rows_d + (size_t)WPB * per_wave_d) + (size_t)wave * per_wave_i;
    double *ox = wd, *oy = ox + cap, *oz = oy + cap, *orr = oz + cap, *oir = orr + cap;
    double *tq = wd + list_d;                                         // [cap][EF][4]: T_f = (Tx Ty Tz T3) of every own bond
    double *stage = tq + tq_d;
    double *zq = stage + (Cfg::STAGE - 4);                            // a quad of zeros (read by the wide windows only)
    const unsigned stage_a = f3_lds_addr(stage), tq_a = f3_lds_addr(tq), zq_a = f3_lds_addr(zq);
    int *oparent = wi, *oshift = wi + cap, *noff = wi + 2 * cap, *nbase = noff + cap + 1, *so = nbase + cap + 1;
    int *osbp = so + (UF3_MAX_SPECIES + 2);                           // first window row of every own bond
    int *ospoff = osbp + cap;                     // [cap][S + 1] (last: the only array whose place depends on S)
    const int sp_stride = S + 1;
    unsigned short *fsrc_l = (unsigned short *)((int *)(rows_lds + rows_d + (size_t)WPB * per_wave_d) + (((size_t)WPB * per_wave_i + 3) & ~(size_t)3));

    for (int q = tid; q < (int)rows_d; q += WPB * WAVE) rows_lds[q] = A.rows[q];
    for (int q = tid; q < A.n_fsrc / 2; q += WPB * WAVE) ((int *)fsrc_l)[q] = ((const int *)A.fsrc)[q];
    if (e_lds) { for (int q = tid; q < F; q += WPB * WAVE) erow[q] = 0.0; }
    for (int q = lane; q < (int)stage_d; q += WAVE) stage[q] = 0.0;
    for (int q = lane; q < (int)tq_d; q += WAVE) tq[q] = 0.0;
    __syncthreads();

    // ---- per-lane constants of the W window: lanes 0-31 hold the sums (x, y) of a position, lanes 32-63 (z, plain); a lane
    // serves NR positions, 32 apart --------------------------------------------------------------------------------------
    const int ext_p = A.ext_p, ext_n = A.ext_n, lo_n = A.lo_n, lo_p = A.lo_p, npos = ext_p * ext_n;
    const int half = lane >> 5;
    int p_lane[NR], n_lane[NR], qn_lane[NR], n32_lane[NR], n32h_lane[NR], p8_lane[NR], qn8_lane[NR], tp_lane[NR];
    const int pr_rows = A.pr_rows;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        // round r holds the rows r * pr_rows ... of the summed leg: local position (row, n) = lane & 31
        const int pl = (lane & 31) / ext_n, p = r * pr_rows + pl;
        const bool on = pl < pr_rows && p < ext_p;
        p_lane[r] = on ? p : 0;
        n_lane[r] = on ? (lane & 31) - pl * ext_n : -(1 << 20);            // (idle positions always read zeros)
        qn_lane[r] = on ? n_lane[r] : RS_C - 1;                            // (... a centre-role record's zero padding)
        n32_lane[r] = n_lane[r] * 32;
        n32h_lane[r] = n32_lane[r] + 16 * half;
        p8_lane[r] = 8 * p_lane[r];                                        // byte offsets of stage 1's reads: a record's bond value,
        qn8_lane[r] = 8 * qn_lane[r];                                      // its n-leg value, the partner's T pair of this half
        tp_lane[r] = 32 * p_lane[r] + 16 * half;
    }
    (void)npos;
    const int sbn_max = ext_n > 4 ? ext_n - 4 : 0, sbp_max = ext_p > 4 ? ext_p - 4 : 0;
    const Feat3Leg leg_p = A.leg_p, leg_n = A.leg_n;
    // rounds that hold rows of a bond whose four functions start at window row sb (all of them when the window has <= 4 rows)
    auto rounds_of = [&](int sb) {
        if (EF <= 4) return (1 << NR) - 1;
        const int r0 = sb / pr_rows, r1 = min(sb + 3, ext_p - 1) / pr_rows;
        return ((2 << r1) - 1) & ~((1 << r0) - 1);
    };

    const int bid = (blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
    const int block_first = bid * A.atoms_per_block;
    const int block_end = min(block_first + A.atoms_per_block, A.natoms);
    int erow_frame = -1;
    for (int m0 = block_first; m0 < block_end; m0 += WPB) {
        const int m = m0 + wave;
        const bool active = m < block_end;
        // the atom's scalars with the workgroup's energy-row check, one wait for all (an idle wave of the last round asks for the
        // block's last atom: nothing past the end of an array)
        const int mc = CH_OWN ? min(m, block_end - 1) : m;
        int fr_c = 0, n_own_c = 0;
        if (CH_OWN) { fr_c = load_const(A.frame_of + mc); n_own_c = load_const(A.n3.cnt + mc); }
        if (e_lds) {
            int f_first = load_const(A.frame_of + m0);
            if (CH_OWN) asm volatile("" : "+s"(fr_c), "+s"(n_own_c), "+s"(f_first));
            if (f_first != erow_frame) {
                __syncthreads();
                if (erow_frame >= 0)
                    for (int q = tid; q < F; q += WPB * WAVE) {
                        double v = erow[q];
                        if (v != 0.0) { unsafeAtomicAdd(A.x_e + (size_t)erow_frame * F + q, v); erow[q] = 0.0; }
                    }
                __syncthreads();
                erow_frame = f_first;
            }
        }
        if (!active) continue;
        const int fr = CH_OWN ? fr_c : load_const(A.frame_of + m);
        const int sm = ((const __attribute__((address_space(4))) signed char *)(unsigned long long)A.spec)[m];
        ESink es;
        es.lds = erow; es.glob = WANT_E ? A.x_e + (size_t)fr * F : nullptr; es.direct = !e_lds || (fr != erow_frame);

        // ---- own 3-body list -> LDS; species offsets of the neighbours' lists ----------------------------------------
        const int n_own = CH_OWN ? n_own_c : load_const(A.n3.cnt + m);
        auto own_entry = [&](int e, const N3Entry &en) {
            ox[e] = en.dx; oy[e] = en.dy; oz[e] = en.dz; orr[e] = en.r; oir[e] = 1.0 / en.r;
            int s0, s1, s2;
            unpack3(en.shiftc, s0, s1, s2);
            oparent[e] = en.parent; oshift[e] = pack3(-s0, -s1, -s2);      // (m's image as the neighbour's list names it)
        };
        // the neighbour's row of species offsets: all nine words of the row are there whatever S is, and are asked for together
        // (S afresh per atom: as loop invariants the nine compares below are kept in nine scalar pairs, and spilled)
        int s_row = S;
        if (CH_ROWS) asm volatile("" : "+s"(s_row));
        auto own_row = [&](int e, int parent) {
            const int *src = A.n3.spoff + (size_t)parent * (UF3_MAX_SPECIES + 1);
            if (CH_ROWS) {
                int w[UF3_MAX_SPECIES + 1];
#pragma unroll
                for (int sp = 0; sp <= UF3_MAX_SPECIES; sp++) w[sp] = src[sp];
                // (all nine here, in front of the first store: left alone the compiler sinks each load to the store that uses it,
                // a wait apiece)
                static_assert(UF3_MAX_SPECIES == 8, "nine words a row");
                asm volatile("" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]), "+v"(w[4]), "+v"(w[5]), "+v"(w[6]), "+v"(w[7]), "+v"(w[8]));
#pragma unroll
                for (int sp = 0; sp <= UF3_MAX_SPECIES; sp++) if (sp <= s_row) ospoff[e * (S + 1) + sp] = w[sp];
            } else {
                for (int sp = 0; sp <= S; sp++) ospoff[e * (S + 1) + sp] = src[sp];
            }
        };
        if (CH_OWN) {
            // the first 64 entries and the atom's own row in one group with its species byte (asked for a few lines up, behind
            // the test for an idle wave), none of them waited for before all are out, and asked for before the count is known: the slots m * ent_stride ... + cap are the atom's (ent_stride >= cap), and what a lane at
            // or past n_own receives is looked at by nothing.  Every lane asks -- lanes past the capacity and past S for the last
            // slot and word again -- so there is no masked region between the loads.
            // (the atom's offsets and the lane afresh per atom: what is derived from them here is made here, not hoisted into
            // registers that live across the atom loop -- with them hoisted the one-round instances spill vector registers, as the
            // parent did for a hoisted per-lane address of its own.  DESIGN.md section 3.6 shows what each tie buys in the listing.)
            size_t own_at = (size_t)m * ent_stride, so_at = (size_t)m * (UF3_MAX_SPECIES + 1);
            int ln = lane;
            asm volatile("" : "+s"(own_at), "+s"(so_at), "+v"(ln));
            const N3Entry *own = A.n3.ent + own_at;
            const N3Entry en = own[(unsigned)min(ln, cap - 1)];
            const int so_v = A.n3.spoff[so_at + (unsigned)min(ln, S)];
            wave_sync();
            if (ln < n_own) own_entry(ln, en);
            if (ln <= S) so[ln] = so_v;
            for (int e = ln + WAVE; e < n_own; e += WAVE) own_entry(e, own[(unsigned)e]);
            if (ln < n_own) own_row(ln, en.parent);
            wave_sync();
            for (int e = ln + WAVE; e < n_own; e += WAVE) own_row(e, oparent[e]);
        } else {
            wave_sync();
            for (int e = lane; e < n_own; e += WAVE) own_entry(e, A.n3.ent[(size_t)m * ent_stride + e]);
            if (lane <= S) so[lane] = A.n3.spoff[(size_t)m * (UF3_MAX_SPECIES + 1) + lane];
            wave_sync();
            for (int e = lane; e < n_own; e += WAVE) own_row(e, oparent[e]);
        }
        // ---- T_f of every own bond: rows over the whole window of the centre legs, zero where the bond's four functions are
        // not (and all zero when the bond is outside the legs' range) -------------------------------------------------------
        for (int e = lane; e < n_own; e += WAVE) {
            const double r = F3_LIST(orr, e);
            double v[4] = {0, 0, 0, 0}, d[4] = {0, 0, 0, 0};
            int sbp = 0;
            if (r > leg_p.t0 && r < leg_p.tlast && !UF3_SKIP(32)) {
                const int iv = f3_eval<true, NFP>(rows, leg_p, r, v, d);
                sbp = max(0, min(sbp_max, iv - 3 - lo_p));
            }
            if (EF > 4) osbp[e] = sbp;
            const double ir = F3_LIST(oir, e), ux = F3_LIST(ox, e) * ir, uy = F3_LIST(oy, e) * ir, uz = F3_LIST(oz, e) * ir;
            double *dst = tq + (size_t)e * EF * 4;
            if (EF > 4) {
#pragma unroll
                for (int q = 0; q < EF; q++) { *(double2 *)(dst + 4 * q) = double2{0.0, 0.0}; *(double2 *)(dst + 4 * q + 2) = double2{0.0, 0.0}; }
                dst += 4 * sbp;
            }
#pragma unroll
            for (int q = 0; q < (EF < 4 ? EF : 4); q++) {
                *(double2 *)(dst + 4 * q) = double2{ux * d[q], uy * d[q]};
                *(double2 *)(dst + 4 * q + 2) = double2{uz * d[q], v[q]};
            }
        }
        wave_sync();

        for (int t = 0; t < n_trios; t++) {
            const TrioDev *td = A.trios + t;
            typedef int int8_v __attribute__((ext_vector_type(8)));
            const int8_v hv = *(const __attribute__((address_space(4))) int8_v *)(unsigned long long)&td->head;
            // (the block's fold table is asked for at the block's top and held in a scalar down to the fold, which no longer
            // waits.  The compiler still issues the load behind the head's wait -- two waits in a row here, not one: DESIGN.md
            // section 3.6)
            int t_fs = CH_FSRC ? load_const(A.trio_fsrc + t) : 0;
            const int t_ncol = hv[2], t_sc = hv[3], t_sa = hv[4], t_sb = hv[5], t_col = hv[6];
            if (CH_FSRC) asm volatile("" : "+s"(t_fs) : "s"(t_sc));
            const bool centre = t_sc == sm, nbr = t_sa == sm || t_sb == sm;
            if (!centre && !nbr) { zero_rows(A.x_f, m, A.ld, t_col, t_ncol); continue; }
            const bool tr = t_sa != t_sb && sm == t_sb;              // transposed: the fixed bond sits on leg m

            double xacc[NR][EF][2], ws[NR][2];
#pragma unroll
            for (int r = 0; r < NR; r++) {
                ws[r][0] = ws[r][1] = 0.0;
#pragma unroll
                for (int q = 0; q < EF; q++) { xacc[r][q][0] = xacc[r][q][1] = 0.0; }
            }
            int cur = -1;                                           // the bond whose W is being summed (own-list index)

            // stage 2: the open bond's W into the rows of the window.  Lower half: rows (x, y) += (Tx, Ty) W_plain + T3 (W_x, W_y);
            // upper half: rows (z, energy) += (Tz, T3) W_plain + T3 (W_z, 0) -- the energy row from the centre role only.
            int wmask = 0;                                          // rounds that took records since the last flush
            auto flush = [&](auto role) {
                constexpr bool IS_C = decltype(role)::value;        // the centre role's flush: the energy row takes part
                if (cur < 0 || UF3_SKIP(2)) return;
                const double *tc = tq + (size_t)cur * EF * 4;
                // (wide windows: only the rounds that were summed into)
                F3Pair tv[EF];
                double t3[EF];
#pragma unroll
                for (int q = 0; q < EF; q++) {
                    tv[q] = *(F3LdsPairs)(const F3Pair *)(tc + 4 * q + 2 * half); t3[q] = ((F3TripReads)tc)[4 * q + 3];
                }
#pragma unroll
                for (int r = 0; r < NR; r++) {
                    if (EF > 4 && !((wmask >> r) & 1)) continue;
                    const int lo = __double2loint(ws[r][1]), hi = __double2hiint(ws[r][1]);
                    const auto r0 = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
                    const auto r1 = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
                    const double wpl = __hiloint2double(r1[1], r0[1]);        // W_plain (the upper half's second sum) in every lane
                    // (the swap's other result keeps the lower half's own second sum in the lower half: ws[r][1] itself is dead from
                    // here on -- it is zeroed below -- and the swap takes one copy per dword instead of two)
                    const double wlo = __hiloint2double(r1[0], r0[0]);
#pragma unroll
                    for (int q = 0; q < EF; q++) xacc[r][q][0] = fma(tv[q].x, wpl, fma(t3[q], ws[r][0], xacc[r][q][0]));
                    // the second chain by halves, as exec masks instead of selected zeros: T3 (W_y) belongs to the lower half only (the
                    // upper half's second sum IS W_plain), T W_plain to both halves in the centre role (Ty | the energy row) and to the
                    // lower half only in the neighbour role.  Inner term first, as ever.
                    if (!half) {
#pragma unroll
                        for (int q = 0; q < EF; q++) {
                            xacc[r][q][1] = fma(t3[q], wlo, xacc[r][q][1]);
                            if (!IS_C) xacc[r][q][1] = fma(tv[q].y, wpl, xacc[r][q][1]);
                        }
                    }
                    if (IS_C) {
#pragma unroll
                        for (int q = 0; q < EF; q++) xacc[r][q][1] = fma(tv[q].y, wpl, xacc[r][q][1]);
                    }
                    ws[r][0] = ws[r][1] = 0.0;
                }
                wmask = 0;
            };

            // ---- centre role: m centres (f, g), f on the fixed leg.  Items p = fi * nG + gi, one per lane and stage slot (not
            // compacted: a void item is a record of zeros); the records of a fixed bond are a run of slots and the T rows of
            // their partners g a run of the table: stage 1 reads both at constant offsets from the run's first record.
            if (centre && !UF3_SKIP(4)) {
                const int fs = tr ? t_sb : t_sa, gs = tr ? t_sa : t_sb;
                const int f_lo = so[fs], nF = so[fs + 1] - f_lo, g_lo = so[gs], nG = so[gs + 1] - g_lo;
                const bool same = t_sa == t_sb;
                const int total = __builtin_amdgcn_readfirstlane(nF * nG);
                const int nGs = __builtin_amdgcn_readfirstlane(nG), f_los = __builtin_amdgcn_readfirstlane(f_lo),
                          g_los = __builtin_amdgcn_readfirstlane(g_lo);
                const float rcp_ng = __builtin_amdgcn_rcpf((float)max(nG, 1));
                for (int p0 = 0; p0 < total; p0 += WAVE) {
                    const int p = p0 + lane;
                    bool valid = p < total;
                    int fi = (int)(((float)p + 0.5f) * rcp_ng);
                    fi -= (fi * nG > p) ? 1 : 0;
                    fi += ((fi + 1) * nG <= p) ? 1 : 0;
                    const int gi = p - fi * nG;
                    valid = valid && (!same || gi > fi);
                    const int f = f_lo + fi, gg = g_lo + gi;
                    double bn[4] = {0, 0, 0, 0}, dum[4];
                    int sbn = 0;
                    if (valid) {
                        const double rf = F3_LIST(orr, f), rg = F3_LIST(orr, gg);
                        const double ex = F3_LIST(ox, gg) - F3_LIST(ox, f), ey = F3_LIST(oy, gg) - F3_LIST(oy, f),
                                     ez = F3_LIST(oz, gg) - F3_LIST(oz, f);
                        const double rn = norm3_leg(ex, ey, ez);
                        valid = (rf > leg_p.t0) & (rf < leg_p.tlast) & (rg > leg_p.t0) & (rg < leg_p.tlast) &
                                (rn > leg_n.t0) & (rn < leg_n.tlast);
                        if (valid && !UF3_SKIP(64)) {
                            const int iv = f3_eval<false>(rows, leg_n, rn, bn, dum);
                            sbn = max(0, min(sbn_max, iv - 3 - lo_n));
                        }
                    }
                    int smask = (1 << NR) - 1;                      // rounds the partners g of this step have rows in
                    if (EF > 4) {
                        const int rm = valid ? rounds_of(osbp[gg]) : 0;
                        smask = 0;
#pragma unroll
                        for (int r = 0; r < NR; r++) smask |= __ballot((rm >> r) & 1) ? (1 << r) : 0;
                    }
                    {
                        double *rp = stage + (size_t)lane * RS_C;
#pragma unroll
                        for (int u = 0; u < RS_C; u += 2) *(double2 *)(rp + u) = double2{0.0, 0.0};
                        if (valid) {
#pragma unroll
                            for (int u = 0; u < 4; u++) rp[sbn + u] = bn[u];
                        }
                    }
                    wave_sync();
                    // rows fi of the item rectangle that this step touches
                    const int p1 = min(total, p0 + WAVE);
                    int fi_s = p0 / nGs;
                    for (int pr = fi_s * nGs; pr < p1 && !UF3_SKIP(1); pr += nGs, fi_s++) {
                        int s0 = max(pr, p0), s1 = min(pr + nGs, p1);               // items of this row inside the step
                        if (same) s0 = max(s0, pr + fi_s + 1);
                        if (s0 >= s1) continue;
                        const int key = f_los + fi_s;
                        if (key != cur) { flush(std::true_type{}); cur = key; }
                        wmask |= smask;
                        unsigned qp = f3_lds_base(stage_a + (s0 - p0) * (RS_C * 8));
                        unsigned tp = f3_lds_base(tq_a + (g_los + (s0 - pr)) * (EF * 32));
                        int cnt = s1 - s0;
                        auto body = [&](auto tag) {
                            constexpr int CNT = decltype(tag)::value;
#pragma unroll
                            for (int r = 0; r < NR; r++) {
                                if (EF > 4 && !((smask >> r) & 1)) continue;
                                double bq[CNT];
                                F3Pair tt[CNT];
#pragma unroll
                                for (int i = 0; i < CNT; i++) {
                                    bq[i] = *(F3TripReads)(qp + qn8_lane[r] + i * RS_C * 8);
                                    tt[i] = *(F3LdsPairs)(tp + tp_lane[r] + i * EF * 32);
                                }
#pragma unroll
                                for (int i = 0; i < CNT; i++) { ws[r][0] = fma(tt[i].x, bq[i], ws[r][0]); ws[r][1] = fma(tt[i].y, bq[i], ws[r][1]); }
                            }
                            qp += CNT * RS_C * 8; tp += CNT * EF * 32; cnt -= CNT;
                            asm("" : "+s"(qp), "+s"(tp));
                        };
                        while (cnt >= 4) body(std::integral_constant<int, 4>{});
                        // (three plain ifs, no else: a body leaves cnt at 0, and the sums stay in the registers of the trip)
                        if (cnt == 3) body(std::integral_constant<int, 3>{});
                        if (cnt == 2) body(std::integral_constant<int, 2>{});
                        if (cnt == 1) body(std::integral_constant<int, 1>{});
                    }
                    wave_sync();
                }
                flush(std::true_type{});
                cur = -1;
            }
            // ---- neighbour role: m is a neighbour of the centre e (fixed bond (m, e)); k runs over e's list.  The valid items of
            // a step are compacted into the stage in order.  A record's header -- its fixed bond and its first n slot -- does not
            // go through LDS memory: the lane that made the record pushes it to the lane of the record's slot (one ds_permute per
            // pass), runs of a fixed bond are one DPP shift, one compare and one ballot over those lanes, and the first n
            // slots of two consecutive records reach stage 1 through ONE v_readlane as scalar operands: no LDS read and no wait in
            // front of a trip's addresses.
            if (nbr && !UF3_SKIP(8)) {
                const int sx = sm == t_sa ? t_sb : t_sa;
                const int rc_lo = so[t_sc], ncen = so[t_sc + 1] - rc_lo;
                int total_n = 0;
                for (int e0 = 0; e0 < ncen; e0 += WAVE) {
                    const int e = e0 + lane;
                    int cnt = 0, base = 0;
                    if (e < ncen) {
                        const int *sp = ospoff + (size_t)(rc_lo + e) * sp_stride;
                        base = sp[sx]; cnt = sp[sx + 1] - base;
                    }
                    const int incl = wave_scan_incl(cnt);
                    if (e < ncen) { noff[e] = total_n + incl - cnt; nbase[e] = base; }
                    total_n += __builtin_amdgcn_readlane(incl, WAVE - 1);
                }
                total_n = __builtin_amdgcn_readfirstlane(total_n);
                if (lane == 0) noff[ncen] = total_n;
                if (NR == 1) {
                    // the records' pads, which stage 1 reads as zeros: the centre role's records and the fold's dump lie over them,
                    // the record stores below never touch them -- once per role
                    static_assert(NR != 1 || RS_N - EFP - 16 == 2, "a neighbour-role record ends in one 16-byte pad");
                    static_assert(NR != 1 || EFP * 8 + 128 + 16 <= RS_N * 8, "the clamped offset (128) must stay inside the record");
                    // (the zero is made here: as a loop invariant the compiler kept four registers of zeros and spilled them)
                    double z;
                    asm volatile("v_mov_b64 %0, 0" : "=v"(z));
                    if (lane < NREC) *(double2 *)(stage + (size_t)lane * RS_N + EFP + 16) = double2{z, z};
                }
                wave_sync();
                for (int p0 = 0; p0 < total_n; p0 += WAVE) {
                    const int q = p0 + lane;
                    bool valid = q < total_n;
                    double pv[4] = {0, 0, 0, 0}, bn[4] = {0, 0, 0, 0}, bd[4] = {0, 0, 0, 0}, a3[3] = {0, 0, 0}, dum[4];
                    int sbn = 0, sbp = 0, e = 0;
                    if (valid) {
                        int lo = 0, hi = ncen - 1;
                        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (noff[mid] <= q) lo = mid; else hi = mid - 1; }
                        e = rc_lo + lo;
                        const int kk = nbase[lo] + (q - noff[lo]);
                        const int pc = oparent[e];
                        const double oex = F3_LIST(ox, e), oey = F3_LIST(oy, e), oez = F3_LIST(oz, e), oer = F3_LIST(orr, e);
                        const N3Entry *kp = A.n3.ent + (size_t)pc * ent_stride + kk;
                        const N3Entry ke = *kp;
                        if (CH_KE) {
                            // parent and shift as one 8-byte load in the group of the entry's other loads, and both compares on
                            // loaded values: no second load, under a mask, behind the wait for the first
                            typedef int int2_v __attribute__((ext_vector_type(2)));
                            const int2_v ps = *(const int2_v *)&kp->parent;
                            valid = !((ps.x == m) & (ps.y == oshift[e]));                      // k is m itself
                        } else {
                            valid = !(ke.parent == m && ke.shiftc == oshift[e]);
                        }
                        const double ex = oex + ke.dx, ey = oey + ke.dy, ez = oez + ke.dz;   // m -> k
                        const double rn = norm3_leg(ex, ey, ez), rk = ke.r;
                        valid = valid & (oer > leg_p.t0) & (oer < leg_p.tlast) & (rk > leg_p.t0) & (rk < leg_p.tlast) &
                                (rn > leg_n.t0) & (rn < leg_n.tlast);
                        if (valid && !UF3_SKIP(64)) {
                            const double in = fast_rcp(rn);
                            a3[0] = ex * in; a3[1] = ey * in; a3[2] = ez * in;
                            const int ivp = f3_eval<false, NFP>(rows, leg_p, rk, pv, dum);
                            sbp = max(0, min(sbp_max, ivp - 3 - lo_p));
                            const int iv = f3_eval<true>(rows, leg_n, rn, bn, bd);
                            sbn = max(0, min(sbn_max, iv - 3 - lo_n));
                        }
                    }
                    const unsigned long long mask = __ballot(valid);
                    const int nv = __popcll(mask), rank = mbcnt(mask);
                    int smask = (1 << NR) - 1;                      // rounds the bonds (e, k) of this step have rows in
                    if (EF > 4) {
                        const int rm = valid ? rounds_of(sbp) : 0;
                        smask = 0;
#pragma unroll
                        for (int r = 0; r < NR; r++) smask |= __ballot((rm >> r) & 1) ? (1 << r) : 0;
                    }
                    for (int sp0 = 0; sp0 < nv; sp0 += NREC) {
                        const int slot = rank - sp0;
                        const bool put = valid && slot >= 0 && slot < NREC;
                        if (put) {
                            double *rp = stage + (size_t)slot * RS_N;
                            if (EF > 4) {
#pragma unroll
                                for (int u = 0; u < EFP; u += 2) *(double2 *)(rp + u) = double2{0.0, 0.0};
#pragma unroll
                                for (int u = 0; u < 4; u++) rp[sbp + u] = pv[u];
                            } else {
                                *(double2 *)rp = double2{pv[0], pv[1]};
                                // (a three-row window: stage 1 reads a record's bond values at p_lane < 3, pv[3] was never evaluated)
                                if (EF == 3) rp[2] = pv[2];
                                else *(double2 *)(rp + 2) = double2{pv[2], pv[3]};
                            }
#pragma unroll
                            for (int u = 0; u < 4; u++) {
                                *(double2 *)(rp + EFP + 4 * u) = double2{a3[0] * bd[u], a3[1] * bd[u]};
                                *(double2 *)(rp + EFP + 2 + 4 * u) = double2{a3[2] * bd[u], bn[u]};
                            }
                        }
                        // the header (fixed bond | 32 x first n slot << 16) to the lane of the slot: one crossbar trip; lanes without a
                        // record push to lane 63, which is no slot
                        static_assert(NREC <= 32 && NREC < WAVE, "lane 63 must stay free of records, lane s + 1 must exist");
                        const int got = __builtin_amdgcn_ds_permute((put ? slot : WAVE - 1) << 2, e | (sbn << 21));
                        const int end = min(NREC, nv - sp0);
                        wave_sync();
                        // lane s: key of record s | first n slots (byte offsets of their quads) of records s and s + 1, 16 bits each
                        const int v_key = got & 0xffff, v_sb1 = got >> 16;
                        const int v_sb = v_sb1 | (__builtin_amdgcn_update_dpp(0, v_sb1, 0x130, 0xf, 0xf, false) << 16);   // wave_shl:1
                        const int v_prev = __builtin_amdgcn_update_dpp(v_key, v_key, 0x138, 0xf, 0xf, false);   // wave_shr:1
                        unsigned long long gm = __ballot(lane < end && (lane == 0 || v_key != v_prev));
                        while (gm && !UF3_SKIP(1)) {
                            const int g0 = __builtin_ctzll(gm);
                            gm &= gm - 1;
                            const int g1 = gm ? __builtin_ctzll(gm) : end;
                            const int key = __builtin_amdgcn_readlane(v_key, g0);
                            if (key != cur) { flush(std::false_type{}); cur = key; }
                            wmask |= smask;
                            unsigned rp = f3_lds_base(stage_a + g0 * (RS_N * 8));
                            int gi = g0, cnt = g1 - g0;
                            auto body = [&](auto tag) {
                                constexpr int CNT = decltype(tag)::value;
                                int sb[CNT];                        // wave-uniform: scalar operands of the subtraction below
#pragma unroll
                                for (int i = 0; i < CNT; i += 2) {
                                    const int w = __builtin_amdgcn_readlane(v_sb, gi + i);
                                    sb[i] = w & 0xffff;
                                    if (i + 1 < CNT) sb[i + 1] = (unsigned)w >> 16;
                                }
#pragma unroll
                                for (int r = 0; r < NR; r++) {
                                    if (EF > 4 && !((smask >> r) & 1)) continue;
                                    double bq[CNT];
                                    F3Pair tt[CNT];
#pragma unroll
                                    for (int i = 0; i < CNT; i++) {
                                        unsigned qa;
                                        if (NR == 1) {
                                            // 32 (n - first slot) + 16 half inside the record's four quads; everything else -- below the
                                            // window (wraps), above it, idle positions -- lands on the record's own pad of zeros
                                            const unsigned off = min((unsigned)(n32h_lane[r] - sb[i]), 128u);
                                            qa = rp + off + (i * RS_N + EFP) * 8;
                                        } else {
                                            const unsigned off_n = (unsigned)(n32_lane[r] - sb[i]);    // 32 (n - first slot)
                                            qa = rp + off_n + (i * RS_N + EFP) * 8 + 16 * half;
                                            qa = off_n < 128u ? qa : zq_a;
                                        }
                                        bq[i] = *(F3TripReads)(rp + p8_lane[r] + i * RS_N * 8);
                                        tt[i] = *(F3LdsPairs)qa;
                                    }
#pragma unroll
                                    for (int i = 0; i < CNT; i++) { ws[r][0] = fma(bq[i], tt[i].x, ws[r][0]); ws[r][1] = fma(bq[i], tt[i].y, ws[r][1]); }
                                }
                                rp += CNT * RS_N * 8; gi += CNT; cnt -= CNT;
                                asm("" : "+s"(rp));
                            };
                            while (cnt >= 4) body(std::integral_constant<int, 4>{});
                            if (cnt == 3) body(std::integral_constant<int, 3>{});
                            if (cnt == 2) body(std::integral_constant<int, 2>{});
                            if (cnt == 1) body(std::integral_constant<int, 1>{});
                        }
                        wave_sync();
                    }
                }
                flush(std::false_type{});
                cur = -1;
            }
            if (UF3_SKIP(16)) continue;
            // ---- fold: the rows of the window -> LDS, the block's columns sum their (one or two) source bins -----------------
            wave_sync();
            const unsigned short *ft = fsrc_l + (CH_FSRC ? t_fs : load_const(A.trio_fsrc + t)) + (size_t)(tr ? 2 * t_ncol : 0);
            if (NR == 1) {
                // (pairs: a lane's two rows side by side -- [half][f][32 positions] x (x, y | z, energy))
#pragma unroll
                for (int q = 0; q < EF; q++)
                    *(double2 *)(stage + (size_t)(((half * EF + q) * 32 + (lane & 31)) * 2)) = double2{xacc[0][q][0], xacc[0][q][1]};
                wave_sync();
                for (int col = lane; col < t_ncol; col += WAVE) {
                    const int s0 = ft[2 * col], s1 = ft[2 * col + 1];
                    F3LdsPairs d0 = (F3LdsPairs)(const F3Pair *)stage, d1 = d0 + EF * 32;
                    const F3Pair a0 = d0[s0], a1 = d0[s1], b0 = d1[s0], b1 = d1[s1];
                    double *dst = A.x_f + (size_t)m * 3 * A.ld + t_col + col;
                    __builtin_nontemporal_store(a0.x + a1.x, dst); __builtin_nontemporal_store(a0.y + a1.y, dst + A.ld);
                    __builtin_nontemporal_store(b0.x + b1.x, dst + 2 * (size_t)A.ld);
                    if (WANT_E) es.add(t_col + col, b0.y + b1.y);
                }
                wave_sync();
            } else {
                // one component of each half at a time -- (x | z), then (y | energy): two buffers [f][32 NR positions] of doubles, a
                // zero behind each for the second source a column may not have
                constexpr int BUF = EF * PS + 2;
#pragma unroll
                for (int k = 0; k < 2; k++) {
#pragma unroll
                    for (int r = 0; r < NR; r++)
#pragma unroll
                        for (int q = 0; q < EF; q++) stage[half * BUF + q * PS + r * 32 + (lane & 31)] = xacc[r][q][k];
                    if (lane == 0 || lane == 32) stage[half * BUF + EF * PS] = 0.0;
                    wave_sync();
                    for (int col = lane; col < t_ncol; col += WAVE) {
                        const int s0 = ft[2 * col], s1 = ft[2 * col + 1];
                        F3LdsDoubles da = (F3LdsDoubles)stage, db = da + BUF;
                        const double va = da[s0] + da[s1];
                        __builtin_nontemporal_store(va, A.x_f + ((size_t)m * 3 + k) * A.ld + t_col + col);
                        if (k == 0 || WANT_E) {
                            const double vb = db[s0] + db[s1];
                            if (k == 0) __builtin_nontemporal_store(vb, A.x_f + ((size_t)m * 3 + 2) * A.ld + t_col + col);
                            else es.add(t_col + col, vb);
                        }
                    }
                    wave_sync();
                }
            }
        }
    }
    if (e_lds) {
        __syncthreads();
        if (erow_frame >= 0)
            for (int q = tid; q < F; q += WPB * WAVE) {
                double v = erow[q];
                if (v != 0.0) unsafeAtomicAdd(A.x_e + (size_t)erow_frame * F + q, v);
            }
    }
}
#undef F3_LIST
