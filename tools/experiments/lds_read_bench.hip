// LDS read throughput on gfx950 for the access shapes of k_featurize3's stage 1: how many cycles of the CU's LDS does one
// wave-instruction take -- full-wave distinct addresses, broadcasts (3 or 9 distinct addresses per wave), and reads with part
// of the lanes masked off?  16 waves per CU (1024 threads), every wave issues independent reads back to back.
// Second table (kg): RATES -- groups of 8 values issued back to back with ONE wait per group, as a stage-1 trip does, at 16 and at
// 8 waves per CU: a two-address ds_read2_b64 against two ds_read_b64 of the same addresses, in the shapes of the trips' and the
// flush's paired reads, and the b64 / b128 shapes of the first table again.
//     hipcc --offload-arch=gfx950 -O3 -w lds_read_bench.hip -o lds_read_bench && ./lds_read_bench [first|rates|wrapped ...]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
typedef double __attribute__((ext_vector_type(2))) d2;
template <int MODE>
__global__ void __launch_bounds__(1024) k(unsigned long long *cyc, double *sink, int iters) {
    __shared__ __align__(16) double buf[8192];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = t; i < 8192; i += 1024) buf[i] = 1e-300 * i;
    __syncthreads();
    const int j = (lane & 31) / 9, n = (lane & 31) % 9, half = lane >> 5;
    int a;                                           // element index
    bool on = true;
    if (MODE == 0) a = lane * 2;                     // b128, 64 distinct addresses, conflict free
    if (MODE == 1) a = j * 4 + half * 2;             // b128, 6 distinct addresses (the P pairs of stage 1)
    if (MODE == 2) a = lane;                         // b64, distinct
    if (MODE == 3) a = n;                            // b64, 9 distinct (the Q values of the centre role)
    if (MODE == 4) { a = j * 4 + half * 2; on = n < 4; }        // b128, 24 of 64 lanes active
    if (MODE == 5) { a = lane * 2; on = lane < 16; }            // b128, 16 contiguous lanes active
    if (MODE == 6) a = (n & 3) * 4 + half * 2;       // b128 of quads 32 B apart (neighbour role's clamped quads)
    if (MODE == 7) a = 0;                            // b32 broadcast
    a += wave * 256;
    double acc0 = 0, acc1 = 0, acc2 = 0, acc3 = 0;
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    if (on) {
        for (int i = 0; i < iters; i++) {
            const int o = (i & 7) * 16;
            if (MODE == 2 || MODE == 3) {
                const __attribute__((address_space(3))) double *p = (const __attribute__((address_space(3))) double *)(buf + a + o);
                double x0 = p[0], x1 = p[64], x2 = p[128], x3 = p[192];
                asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));
                acc0 += x0; acc1 += x1; acc2 += x2; acc3 += x3;
            } else if (MODE == 7) {
                const __attribute__((address_space(3))) int *p = (const __attribute__((address_space(3))) int *)(buf + a + o);
                int x0 = p[0], x1 = p[64], x2 = p[128], x3 = p[192];
                asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));
                acc0 += x0; acc1 += x1; acc2 += x2; acc3 += x3;
            } else {
                const d2 *p = (const d2 *)(buf + a + o);
                d2 x0 = __builtin_nontemporal_load(p), x1 = __builtin_nontemporal_load(p + 32), x2 = __builtin_nontemporal_load(p + 64), x3 = __builtin_nontemporal_load(p + 96);
                asm volatile("" : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3));
                acc0 += x0.x; acc1 += x1.y; acc2 += x2.x; acc3 += x3.y;
            }
        }
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    __syncthreads();
    const unsigned long long t2 = __builtin_amdgcn_s_memtime();
    if (t == 0) cyc[blockIdx.x] = t2 - t0;
    (void)t1;
    if (acc0 + acc1 + acc2 + acc3 == 12345.678) sink[0] = acc0;
}
template <int MODE> void run(const char *what) {
    unsigned long long *cyc; double *sink;
    hipMalloc(&cyc, 8 * 256); hipMalloc(&sink, 8);
    const int iters = 4000;
    hipLaunchKernelGGL(k<MODE>, dim3(256), dim3(1024), 0, 0, cyc, sink, iters);
    hipDeviceSynchronize();
    unsigned long long h[256]; hipMemcpy(h, cyc, 8 * 256, hipMemcpyDeviceToHost);
    double avg = 0; for (int i = 0; i < 256; i++) avg += (double)h[i] / 256;
    printf("%-62s %.2f LDS cycles per wave-instruction (16 waves per CU)\n", what, avg / (16.0 * 4 * iters));
    hipFree(cyc); hipFree(sink);
}
// ---- rates: 8 values per group, one wait per group ----------------------------------------------------------------------------
// The instructions are written out (this is a measurement of instructions, not of what the compiler makes of C++): %0 ... the
// destinations, the last operand the per-lane byte address.  offset0 / offset1 of ds_read2_b64 count 8-byte elements, offset bytes.
#define R2(d, o0, o1) "ds_read2_b64 %" #d ", %4 offset0:" #o0 " offset1:" #o1 "\n"
#define R1(d, o) "ds_read_b64 %" #d ", %8 offset:" #o "\n"
#define RQ(d, o) "ds_read_b128 %" #d ", %8 offset:" #o "\n"
#define WAIT0 "s_waitcnt lgkmcnt(0)"
#define OUT4(T) T x0, x1, x2, x3
#define OUT8(T) T x0, x1, x2, x3, x4, x5, x6, x7
#define ASM4(text) asm volatile(text WAIT0 : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3) : "v"(addr))
#define ASM8(text) asm volatile(text WAIT0 : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3), "=&v"(x4), "=&v"(x5), "=&v"(x6), "=&v"(x7) : "v"(addr))
enum { G_B128_64, G_B128_6, G_B64_64, G_B64_9, G_B64_3, G_PAIR_3, G_PAIR_9, G_B64_1, G_PAIR_1, G_TRIP_PAIRS, G_TRIP_SINGLES, G_MODES };
struct GMode { const char *what; int values; int insts; };      // 8-byte values a lane receives, and instructions, per group
static const GMode g_modes[G_MODES] = {
    {"ds_read_b128 x 8, 64 distinct addresses", 16, 8},
    {"ds_read_b128 x 8, 6 distinct addresses (P pairs)", 16, 8},
    {"ds_read_b64 x 8, 64 distinct addresses", 8, 8},
    {"ds_read_b64 x 8, 9 distinct addresses, records 10 doubles apart", 8, 8},
    {"ds_read_b64 x 8, 3 distinct addresses, records 22 doubles apart", 8, 8},
    {"ds_read2_b64 x 4, 3 distinct addresses, offsets 0 / 22", 8, 4},
    {"ds_read2_b64 x 4, 9 distinct addresses, offsets 0 / 10", 8, 4},
    {"ds_read_b64 x 8, one address, offsets 83, 87, ...", 8, 8},
    {"ds_read2_b64 x 4, one address, offsets 83 / 87", 8, 4},
    {"a trip of four as compiled: 2 ds_read2_b64 (0 / 22) + 4 ds_read_b128", 12, 6},
    {"a trip of four, bond values alone: 4 ds_read_b64 + 4 ds_read_b128", 12, 8},
};
typedef float __attribute__((ext_vector_type(4))) q4;            // four dwords: the destination of a paired or a 16-byte read
constexpr int KG_BUF = 10496;                                    // 82 KiB: one workgroup per CU, whatever its size
constexpr int KG_WAVE_D = 512;                                   // doubles of LDS a wave reads in
template <int MODE, int WAVES>
__global__ void __launch_bounds__(WAVES * 64) kg(unsigned long long *cyc, double *sink, int iters) {
    __shared__ __align__(16) double buf[KG_BUF];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    for (int i = t; i < KG_BUF; i += WAVES * 64) buf[i] = 1e-300 * i;
    __syncthreads();
    const int j = (lane & 31) / 9, n = (lane & 31) % 9, half = lane >> 5;
    int a = 0;                                                   // element index; every mode reads below a + 256 (static_asserts in main)
    if (MODE == G_B128_64) a = lane * 2;
    if (MODE == G_B128_6) a = (j % 3) * 4 + half * 2;
    if (MODE == G_B64_64) a = lane;
    if (MODE == G_B64_9 || MODE == G_PAIR_9) a = n;
    if (MODE == G_B64_3 || MODE == G_PAIR_3) a = j % 3;
    if (MODE == G_TRIP_PAIRS || MODE == G_TRIP_SINGLES) a = j % 3;   // (the quads of the trip: 32 n + 16 half bytes behind the bond values)
    a += wave * KG_WAVE_D;
    const unsigned addr0 = (unsigned)(size_t)(const __attribute__((address_space(3))) double *)(buf + a);
    const unsigned qoff = (MODE == G_TRIP_PAIRS || MODE == G_TRIP_SINGLES) ? 32 + (n & 3) * 32 + 16 * half - 8 * (j % 3) : 0;
    float acc = 0;
    __syncthreads();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    for (int i = 0; i < iters; i++) {
        const unsigned addr = addr0 + (i & 7) * 16;
        if (MODE == G_B128_64 || MODE == G_B128_6) {
            OUT8(q4);
            ASM8(RQ(0, 0) RQ(1, 128) RQ(2, 256) RQ(3, 384) RQ(4, 512) RQ(5, 640) RQ(6, 768) RQ(7, 896));
            acc += x0.x + x1.y + x2.z + x3.w + x4.x + x5.y + x6.z + x7.w;
        } else if (MODE == G_B64_64) {
            OUT8(double);
            ASM8(R1(0, 0) R1(1, 64) R1(2, 128) R1(3, 192) R1(4, 256) R1(5, 320) R1(6, 384) R1(7, 448));
            acc += (float)(x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7);
        } else if (MODE == G_B64_9) {
            OUT8(double);
            ASM8(R1(0, 0) R1(1, 80) R1(2, 160) R1(3, 240) R1(4, 320) R1(5, 400) R1(6, 480) R1(7, 560));
            acc += (float)(x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7);
        } else if (MODE == G_B64_3) {
            OUT8(double);
            ASM8(R1(0, 0) R1(1, 176) R1(2, 352) R1(3, 528) R1(4, 704) R1(5, 880) R1(6, 1056) R1(7, 1232));
            acc += (float)(x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7);
        } else if (MODE == G_B64_1) {
            OUT8(double);
            ASM8(R1(0, 664) R1(1, 696) R1(2, 760) R1(3, 792) R1(4, 856) R1(5, 888) R1(6, 952) R1(7, 984));
            acc += (float)(x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7);
        } else if (MODE == G_PAIR_3) {
            OUT4(q4);
            ASM4(R2(0, 0, 22) R2(1, 44, 66) R2(2, 88, 110) R2(3, 132, 154));
            acc += x0.x + x1.y + x2.z + x3.w;
        } else if (MODE == G_PAIR_9) {
            OUT4(q4);
            ASM4(R2(0, 0, 10) R2(1, 20, 30) R2(2, 40, 50) R2(3, 60, 70));
            acc += x0.x + x1.y + x2.z + x3.w;
        } else if (MODE == G_PAIR_1) {
            OUT4(q4);
            ASM4(R2(0, 83, 87) R2(1, 95, 99) R2(2, 107, 111) R2(3, 119, 123));
            acc += x0.x + x1.y + x2.z + x3.w;
        } else if (MODE == G_TRIP_PAIRS) {
            q4 x0, x1, x2, x3, x4, x5;
            asm volatile("ds_read2_b64 %0, %6 offset1:22\n" "ds_read_b128 %2, %7 offset:0\n" "ds_read_b128 %3, %7 offset:176\n"
                         "ds_read2_b64 %1, %6 offset0:44 offset1:66\n" "ds_read_b128 %4, %7 offset:352\n" "ds_read_b128 %5, %7 offset:528\n" WAIT0
                         : "=&v"(x0), "=&v"(x1), "=&v"(x2), "=&v"(x3), "=&v"(x4), "=&v"(x5) : "v"(addr), "v"(addr + qoff));
            acc += x0.x + x1.y + x2.z + x3.w + x4.x + x5.y;
        } else if (MODE == G_TRIP_SINGLES) {
            double b0, b1, b2, b3; q4 x2, x3, x4, x5;
            asm volatile("ds_read_b64 %0, %8\n" "ds_read_b128 %4, %9 offset:0\n" "ds_read_b64 %1, %8 offset:176\n" "ds_read_b128 %5, %9 offset:176\n"
                         "ds_read_b64 %2, %8 offset:352\n" "ds_read_b128 %6, %9 offset:352\n" "ds_read_b64 %3, %8 offset:528\n" "ds_read_b128 %7, %9 offset:528\n" WAIT0
                         : "=&v"(b0), "=&v"(b1), "=&v"(b2), "=&v"(b3), "=&v"(x2), "=&v"(x3), "=&v"(x4), "=&v"(x5) : "v"(addr), "v"(addr + qoff));
            acc += (float)(b0 + b1 + b2 + b3) + x2.z + x3.w + x4.x + x5.y;
        }
    }
    __syncthreads();
    const unsigned long long t2 = __builtin_amdgcn_s_memtime();
    if (t == 0) cyc[blockIdx.x] = t2 - t0;
    if (acc == 12345.678f) sink[0] = acc;
}
template <int MODE, int WAVES> void run_rate() {
    unsigned long long *cyc; double *sink;
    hipMalloc(&cyc, 8 * 256); hipMalloc(&sink, 8);
    const int iters = 4000;
    hipLaunchKernelGGL((kg<MODE, WAVES>), dim3(256), dim3(WAVES * 64), 0, 0, cyc, sink, iters);
    hipDeviceSynchronize();
    unsigned long long h[256]; hipMemcpy(h, cyc, 8 * 256, hipMemcpyDeviceToHost);
    double avg = 0; for (int i = 0; i < 256; i++) avg += (double)h[i] / 256;
    const double per_group = avg / ((double)WAVES * iters);
    printf("%-72s %2d waves per CU: %6.2f cycles per wave-instruction, %6.2f per 8-byte value, %7.2f per group of %d values\n",
           g_modes[MODE].what, WAVES, per_group / g_modes[MODE].insts, per_group / g_modes[MODE].values, per_group, g_modes[MODE].values);
    hipFree(cyc); hipFree(sink);
}
template <int MODE> void run_rates() {
    run_rate<MODE, 16>(); run_rate<MODE, 8>();
    if constexpr (MODE + 1 < G_MODES) run_rates<MODE + 1>();
}
// the farthest byte a lane reads lies inside its wave's part of the buffer: address (<= 63 elements, or 2 + a quad offset) + (i & 7) * 16
// + the largest immediate offset + the access width
static_assert(63 * 16 + 7 * 16 + 896 + 16 <= KG_WAVE_D * 8, "b128, 64 addresses");
static_assert(8 * 8 + 7 * 16 + 1232 + 8 <= KG_WAVE_D * 8 && 8 * 8 + 7 * 16 + 154 * 8 + 8 <= KG_WAVE_D * 8, "b64 and pairs");
static_assert(2 * 8 + 32 + 3 * 32 + 16 + 7 * 16 + 528 + 16 <= KG_WAVE_D * 8, "the trip's quads");
static_assert(16 * KG_WAVE_D <= KG_BUF, "16 waves");
// does a DS read beyond the workgroup's allocation return zero?
__global__ void oob(double *out) {
    extern __shared__ double dyn[];
    dyn[threadIdx.x] = 7.0;
    __syncthreads();
    const unsigned addr = 0xfffffff0u - 64u * threadIdx.x;                      // "negative" byte offsets
    double v;
    asm volatile("ds_read_b64 %0, %1\n s_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr));
    out[threadIdx.x] = v;
}
int main(int argc, char **argv) {
    auto want = [&](const char *what) { if (argc < 2) return true; for (int i = 1; i < argc; i++) if (!strcmp(argv[i], what)) return true; return false; };
    if (want("first")) {
        run<0>("b128, 64 distinct addresses");
        run<1>("b128, 6 distinct addresses (P pairs: 3 rows x 2 halves)");
        run<6>("b128, 8 distinct addresses 32 B apart");
        run<4>("b128, 6 distinct addresses, 24 of 64 lanes active");
        run<5>("b128, lanes 0-15 active");
        run<2>("b64, 64 distinct addresses");
        run<3>("b64, 9 distinct addresses (Q values)");
        run<7>("b32, one address");
    }
    if (want("rates")) run_rates<0>();
    if (want("wrapped")) {
        double *o; hipMalloc(&o, 64 * 8);
        hipLaunchKernelGGL(oob, dim3(1), dim3(64), 1024, 0, o);
        double h[64]; hipMemcpy(h, o, 64 * 8, hipMemcpyDeviceToHost);
        int nz = 0; for (int i = 0; i < 64; i++) nz += h[i] != 0.0;
        printf("DS reads at wrapped (negative) addresses: %d of 64 lanes non-zero (0 = out-of-range reads return zero)\n", nz);
    }
    return 0;
}
