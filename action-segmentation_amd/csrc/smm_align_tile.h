// smm_align_tile.h -- what the transcript kernels share (smm_align.hip: the best alignment; smm_align_opt.hip: the same with
// optional entries; smm_align_logz.hip, smm_align_opt_logz.hip: the sums over all alignments): the tile geometry of a column, the cells of a column
// that lie on a complete alignment, the prefix-sum phase, and the tests on the bits.  The including unit chooses its tile:
// SMM_ALIGN_THREADS threads, SMM_ALIGN_R positions per thread (odd: the threads' h reads are R doubles apart, which spreads a
// half-wave over all 64 banks).
#pragma once
#include "smm_device.h"
#include "../../include/smmdp.h"

#if !defined(SMM_ALIGN_THREADS) || !defined(SMM_ALIGN_R)
#error "define SMM_ALIGN_THREADS (threads per workgroup) and SMM_ALIGN_R (positions per thread) before this header"
#endif
#define SMM_ALIGN_P (SMM_ALIGN_THREADS * SMM_ALIGN_R)            // positions per tile
#define SMM_ALIGN_DMAX ((SMM_MAX_K_ROWS + SMM_ALIGN_R - 1) / SMM_ALIGN_R * SMM_ALIGN_R)   // distances walked, at most
#define SMM_ALIGN_OFF SMM_ALIGN_DMAX                             // LDS index of the tile's first position
#define SMM_ALIGN_HS (SMM_ALIGN_OFF + SMM_ALIGN_P + 8)           // h values in LDS: halo | tile | the R ahead
#define SMM_ALIGN_LEN (SMM_ALIGN_DMAX + 3 * SMM_ALIGN_R)         // length scores in LDS: index k + R, -inf outside 1 .. kp - 1

static_assert(SMM_ALIGN_R % 2 == 1, "an even stride puts a half-wave's h reads on a quarter of the banks");
static_assert(SMM_MAX_TRANSCRIPT <= SMM_ALIGN_THREADS, "one thread per transcript position checks its tables");

__device__ __forceinline__ double align_max(double a, double b) { return __builtin_fmax(a, b); }

// NaN or +-inf by the bits (exponent all ones)
__device__ __forceinline__ bool align_nonfinite_bits(double x)
{
    int hi = __double2hiint(x);
    asm volatile("" : "+v"(hi));
    return (hi & 0x7ff00000) == 0x7ff00000;
}
// NaN or +inf: what must not enter the DP (-inf is an ordinary "impossible")
__device__ __forceinline__ bool align_bad_bits(double x)
{
    return smm_nan_bits(x) || (align_nonfinite_bits(x) && __double2hiint(x) >= 0);
}

__device__ __forceinline__ double align_wave_max(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = align_max(x, __shfl_xor(x, off));
    return x;
}

__device__ __forceinline__ int align_wave_min(int x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const int y = __shfl_xor(x, off);
        x = y < x ? y : x;
    }
    return x;
}

// the cells of column m that lie on a complete alignment (lo > hi: none)
__device__ __forceinline__ void align_range(int m, int M, int T, int kw, int &lo, int &hi)
{
    const int rest = M - 1 - m;
    const int a = m + 1, b = T - rest * kw;
    const int c = T - rest, d = (m + 1) * kw;
    lo = a > b ? a : b;
    hi = c < d ? c : d;
}

// ... and the positions at which segment m can start: {0} for m = 0, else the cells of column m - 1
__device__ __forceinline__ void align_start_range(int m, int M, int T, int kw, int &lo, int &hi)
{
    lo = hi = 0;
    if (m > 0) align_range(m - 1, M, T, kw, lo, hi);
}

// ... with optional entries (smm_align_opt.hip, smm_align_opt_logz.hip): nb / na: mandatory entries before / after m
__device__ __forceinline__ void align_opt_range(int m, int M, int T, int kw, int nb, int na, int &lo, int &hi)
{
    const int a = nb + 1, b = T - (M - 1 - m) * kw;
    const int c = T - na, d = (m + 1) * kw;
    lo = a > b ? a : b;
    hi = c < d ? c : d;
}

// Prefix sums of one video: tiles of `rows` frames through LDS (s_h: SMM_ALIGN_HS doubles), lane c adds class c serially,
// cum[c][n] class-major [C][T+1].  Every thread of the workgroup calls it; returns true in the threads whose class total is not
// finite.  The caller puts a barrier behind it before cum is read.
__device__ __forceinline__ bool align_prefix_sums(const double *elp, double *cum, int C, int cm, int T, double *s_h, int tid)
{
    const size_t T1 = (size_t)T + 1;
    const int ld = cm + 1;                                 // row stride in LDS: odd, so the transposing reads spread over the banks
    const int rows = SMM_ALIGN_HS / ld;
    double run = 0.0;
    if (tid < C) cum[(size_t)tid * T1] = 0.0;
    for (int f0 = 0; f0 < T; f0 += rows) {
        const int nr = T - f0 < rows ? T - f0 : rows;
        __syncthreads();
        for (int e = tid; e < nr * cm; e += SMM_ALIGN_THREADS) {
            const int r = e / cm, c = e - r * cm;
            s_h[r * ld + c] = elp[(size_t)f0 * cm + e];
        }
        __syncthreads();
        if (tid < C) {
#pragma unroll 8
            for (int r = 0; r < nr; ++r) {
                run = run + s_h[r * ld + tid];
                s_h[r * ld + tid] = run;
            }
        }
        __syncthreads();
        for (int e = tid; e < nr * C; e += SMM_ALIGN_THREADS) {
            const int c = e / nr, r = e - c * nr;
            cum[(size_t)c * T1 + f0 + 1 + r] = s_h[r * ld + c];
        }
    }
    return tid < C && align_nonfinite_bits(run);
}
