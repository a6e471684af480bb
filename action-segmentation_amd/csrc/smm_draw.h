// smm_draw.h -- what the backward samplers share (smm_sample.hip: the unconstrained posterior; smm_align_graph_sample.hip: the
// transcript-graph posterior): the counter-based random numbers and one draw of a wave among the candidates its lanes hold.
//
// Random numbers: Philox4x32-10 keyed by the seed; counter = (decision number, sample, video, sampler).  The last word tells the
// samplers apart (0: smm_sample.hip, 1: smm_align_graph_sample.hip), so that under one seed they never share a stream.  A
// sample's draws depend on (seed, video, sample) only: not on the grid, on n_samples or on the order the waves run in.  u takes
// 53 random bits.
//
// A draw: lane l holds candidates l, l + 64, ... (NI per lane), wave max, fp64 exp(w - max), a wave inclusive prefix sum (DPP
// within rows of 16, row offsets by readlane), then the first candidate whose prefix exceeds u * total (inverse CDF).  Nothing
// goes through LDS.
#pragma once
#include "smm_device.h"

struct SmmPhilox { uint32_t v[4]; };

__device__ __forceinline__ SmmPhilox smm_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
        const uint32_t lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
        const uint32_t n0 = hi1 ^ c1 ^ k0, n2 = hi0 ^ c3 ^ k1;
        c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    SmmPhilox r;
    r.v[0] = c0; r.v[1] = c1; r.v[2] = c2; r.v[3] = c3;
    return r;
}

// uniform in [0, 1) with 53 random bits, for decision `dec` of the stream (seed, video, sample) of sampler `which`
__device__ __forceinline__ double smm_uniform53(uint64_t seed, int vid, int smp, uint32_t dec, uint32_t which)
{
    const SmmPhilox r = smm_philox4x32_10(dec, (uint32_t)smp, (uint32_t)vid, which, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t bits = ((uint64_t)(r.v[0] >> 5) << 26) | (uint64_t)(r.v[1] >> 6);
    return (double)bits * 0x1.0p-53;
}

// lane i <- lane i - n of its row of 16, 0 where that lies outside the row
template <int N>
__device__ __forceinline__ double smm_row_shr0(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), SMM_DPP_ROW_SHR(N), 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), SMM_DPP_ROW_SHR(N), 0xf, 0xf, false);
    return smm_pack(lo, hi);
}

// inclusive prefix sum over the wave: within each row of 16 by DPP shifts, then the totals of the rows in front by readlane
__device__ __forceinline__ double smm_wave_incl_sum(double x, int lane)
{
    x += smm_row_shr0<1>(x);
    x += smm_row_shr0<2>(x);
    x += smm_row_shr0<4>(x);
    x += smm_row_shr0<8>(x);
    const double r0 = smm_readlane(x, 15), r1 = smm_readlane(x, 31), r2 = smm_readlane(x, 47);
    const int row = lane >> 4;
    const double r01 = r0 + r1;
    const double off = (row == 0) ? 0.0 : (row == 1) ? r0 : (row == 2) ? r01 : r01 + r2;
    return x + off;
}

// One draw among the candidates w[i] of every lane (candidate number i * 64 + lane; -inf = none), probability
// proportional to exp(w).  Returns the candidate number, or -1 when no candidate has a finite weight (or a NaN got in).
template <int NI>
__device__ __forceinline__ int smm_draw(const double (&w)[NI], double u, int lane)
{
    double m = w[0];
#pragma unroll
    for (int i = 1; i < NI; ++i) m = fmax(m, w[i]);
    m = smm_group_max<64>(m);
    if (!(m > SMM_NEG_INF) || m == -SMM_NEG_INF) return -1;
    double e[NI], ls = 0.0;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        e[i] = exp(w[i] - m);                  // (w = -inf: 0)
        ls += e[i];
    }
    const double incl = smm_wave_incl_sum(ls, lane);
    const double tot = smm_readlane(incl, 63);
    if (!(tot >= 1.0) || !(tot < 1e300)) return -1;      // (the maximal candidate alone gives 1; NaN fails both)
    const double tgt = u * tot;
    uint64_t mask = __ballot(incl > tgt);
    if (mask == 0) {                                     // (rounding: u * total came out as total -- the last lane with mass)
        const uint64_t nz = __ballot(ls > 0.0);
        mask = nz ? (1ull << (63 - __builtin_clzll(nz))) : 0ull;
    }
    if (mask == 0) return -1;
    const int L = __builtin_ctzll(mask);
    // in every lane: the first of its own candidates whose running prefix exceeds the target (the last with mass otherwise)
    double run = incl - ls;
    int pick = -1, lastnz = -1;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
        run += e[i];
        if (e[i] > 0.0) lastnz = i;
        if (pick < 0 && e[i] > 0.0 && run > tgt) pick = i;
    }
    if (pick < 0) pick = lastnz;
    const int pi = __builtin_amdgcn_readlane(pick, L);
    return pi < 0 ? -1 : pi * 64 + L;
}

__device__ __forceinline__ int64_t smm_gid(const int64_t *cmap, int c) { return cmap ? cmap[c] : (int64_t)c; }
