// smm_flow.hip -- the NICE additive coupling flow in front of the emission scorer, forward and backward, and the
// gradient of the emission scores with respect to the features, which the backward pass starts from.
//
// y = flow(x), row by row.  Coupling layer i splits a row into halves (h1, h2) of D/2; for even i the passive half is h1 and
// the active one h2, for odd i the other way round; the passive half is copied and the active half becomes
// active + t_i(passive), t_i a ReLU MLP: in_layer (D/2 -> H), `hidden_layers` layers H -> H, out_layer (H -> D/2), ReLU behind
// every layer but the last.  The Jacobian is unit triangular: log det = 0.
//
// One workgroup of four waves owns a tile of 16 x strips rows and carries it through every coupling layer in LDS: the row tile
// (sH) and the MLP's activations (sA) never leave the chip.  Every product runs on v_mfma_f32_16x16x4_f32: inputs,
// accumulation, bias, ReLU and the residual add are fp32.  An accumulator starts at the bias and takes the products in
// ascending k, so a row's result is ONE k-ordered fma chain whatever its place in the tile or the launch; k and n are padded
// with zeros up to the MFMA tile (fma(0, 0, acc) = acc).  A weight matrix is staged through LDS in slabs of `slab_rows` k-rows
// (sW); all four waves read a slab, each for its own (row strip, column tiles).
//
// Backward: activations are not stored.  The tile's forward pass is run again (x -> y in sH), keeping each coupling layer's
// active half as it came in (couple_layers x rows x D/2 floats of LDS); then the layers are walked from the last to the first:
// the layer's MLP is computed again from its passive half, its activations left in LDS for the chain rule, and the active half
// is put back -- every layer sees the forward pass's own bits.  Where no tile with that buffer fits the LDS (D = 512 with H = 256
// and two hidden layers from three coupling layers on, or with H = 100 from five on) the halves go to the workgroup's own
// slice of the caller's scratch instead: every element is written and read back by the same lane.  The flow's inverse
// (active -= t_i(passive)) would need no buffer, but recovers fl(fl(a + t) - t), an ulp off a, and carries that error into the
// layers below; it is not used.
// Weight gradients of a tile are MFMA products over the tile's rows (fp32), added as fp64 into the workgroup's own partial
// buffer: workgroup g takes tiles g, g + grid, ... and every element of its partial is only ever touched by one fixed lane,
// so there are no atomics and no order of arrival; smm_flow_reduce_kernel adds the partials in workgroup order.
#include <hip/hip_runtime.h>
#include <algorithm>
#include "smm_launch.h"

typedef float smm_f32x4 __attribute__((ext_vector_type(4)));

#define SMM_FLOW_JMAX 16            // column tiles of 16 per wave at most: H <= 256 with one wave per row strip
#define SMM_FLOW_LDS_MAX (160 * 1024)

// row strides (floats).  Tile and activations: 4 x odd, so the 16 rows of an A fragment start in 16 different bank groups of 4;
// weight slab: 16 mod 64, so the 4 k-rows of a B fragment cover the 64 banks once.
__host__ __device__ static inline int smm_flow_row_stride(int n)
{
    int s = (n + 3) & ~3;
    if (((s >> 2) & 1) == 0) s += 4;
    return s;
}
__host__ __device__ static inline int smm_flow_slab_stride(int np)   // np: a multiple of 16
{
    int s = np;
    while ((s & 63) != 16) s += 16;
    return s;
}
__host__ __device__ static inline size_t smm_flow_layer_params(int dh, int h, int hl)
{
    return (size_t)dh * h + h + (size_t)hl * ((size_t)h * h + h) + (size_t)h * dh + dh;
}

bool smm_flow_plan(int64_t n_rows, int d, int h, int hidden_layers, int couple_layers, bool bwd, SmmFlowPlan *out)
{
    const int dh = d / 2, np = std::max((h + 15) & ~15, (dh + 15) & ~15);
    const size_t s_h = smm_flow_row_stride(d), s_a = smm_flow_row_stride((h + 15) & ~15), s_w = smm_flow_slab_stride(np);
    // backward: first the tiles that keep every coupling layer's active half in LDS (keep = 1), then, where none fits, the ones
    // that keep them in the workgroup's slice of the scratch (keep = 2)
    const int tries[8][3] = {{4, 16, 1}, {2, 16, 1}, {1, 16, 1}, {1, 8, 1}, {4, 16, 0}, {2, 16, 0}, {1, 16, 0}, {1, 8, 0}};
    for (const auto &t : tries) {
        if (!bwd && t[2]) continue;
        const size_t m = 16 * (size_t)t[0];
        const size_t floats = bwd ? 2 * m * s_h + (size_t)(hidden_layers + 1) * m * s_a + t[1] * s_w + (t[2] ? (size_t)couple_layers * m * dh : 0)
                                  : m * s_h + m * s_a + t[1] * s_w;
        if (floats * sizeof(float) > SMM_FLOW_LDS_MAX) continue;
        out->strips = t[0];
        out->slab_rows = t[1];
        out->keep = bwd ? (t[2] ? 1 : 2) : 0;
        out->keep_floats = out->keep == 2 ? (size_t)couple_layers * m * dh : 0;
        out->lds_bytes = floats * sizeof(float);
        out->n_params = (size_t)couple_layers * smm_flow_layer_params(dh, h, hidden_layers);
        const int64_t n_tiles = (n_rows + (int64_t)m - 1) / (int64_t)m;
        if (n_tiles > 0x7fffffff) return false;
        out->n_tiles = (int32_t)n_tiles;
        int64_t grid = std::min<int64_t>(n_tiles, bwd ? 256 : (1 << 20));
        if (bwd)      // the partials: at most 256 MB, one workgroup at the least
            grid = std::max<int64_t>(1, std::min<int64_t>(grid, (int64_t)((size_t)256 << 20) / (int64_t)(sizeof(double) * out->n_params)));
        out->grid = (int32_t)grid;
        return true;
    }
    return false;
}

// the wave's number as a scalar: the compiler cannot tell that threadIdx.x >> 6 is the same on every lane, and would put every
// wave-level decision (which strip, which column tiles) under an execution mask
__device__ __forceinline__ int smm_flow_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }

enum { SMM_FLOW_RELU = 0, SMM_FLOW_ADD = 1, SMM_FLOW_MASK = 3, SMM_FLOW_SKIP = 4 };

// Out[rows][n] (op)= sum_k In[rows][k] B[k][n] (+ bias[n]), k < K, n < N, over the whole tile.
//   TRANS = false: B[k][n] = W[k * N + n]   (a linear layer, W its packed [in][out] matrix)
//   TRANS = true:  B[k][n] = W[n * K + k]   (the chain rule through it: k runs over the layer's outputs, n over its inputs)
//   RELU: Out = max(acc, 0), every column up to the MFMA tile (the padding comes out 0)      ADD: Out += acc, n < N
//   MASK: Out = acc where Mask > 0, else 0 (ReLU's derivative; Out may be Mask)
// Out may be In: every wave holds its results in registers until all have read their last operand.  Barriers: one before
// the first slab is written (what the caller wrote is visible, what it read from sW is done), one behind every slab, one
// before the results are written.
template <bool TRANS, int MODE>
__device__ __forceinline__ void smm_flow_gemm(const float *sIn, int strideIn, int K, float *sOut, int strideOut, int N,
                                              const float *__restrict__ W, const float *__restrict__ bias,
                                              const float *sMask, int strideMask, float *sW, int strideW, int strips,
                                              int slab_rows)
{
    const int tid = threadIdx.x, wave = smm_flow_wave(), lane = tid & 63;
    const int strip = wave % strips, cg = wave / strips, ncg = 4 / strips;
    const int Np = (N + 15) & ~15, NT = Np >> 4, Kp = (K + 3) & ~3;
    const int lrow = lane & 15, lk = lane >> 4;
    smm_f32x4 acc[SMM_FLOW_JMAX];
#pragma unroll
    for (int j = 0; j < SMM_FLOW_JMAX; ++j) {
        const int n = (cg + j * ncg) * 16 + lrow;
        const float b = (bias != nullptr && n < N) ? bias[n] : 0.f;
        acc[j] = smm_f32x4{b, b, b, b};
    }
    const float *arow = sIn + (size_t)(strip * 16 + lrow) * strideIn;
#pragma nounroll
    for (int k0 = 0; k0 < Kp; k0 += slab_rows) {
        __syncthreads();
        if (!TRANS) {
#pragma nounroll
            for (int kk = wave; kk < slab_rows; kk += 4) {
                const int k = k0 + kk;
#pragma nounroll
                for (int n = lane; n < Np; n += 64) sW[kk * strideW + n] = (k < K && n < N) ? W[(size_t)k * N + n] : 0.f;
            }
        } else {
            const int kk = tid & 15, k = k0 + kk;                 // (consecutive lanes: consecutive k, contiguous in W)
            if (kk < slab_rows)
#pragma nounroll
                for (int n = tid >> 4; n < Np; n += 16) sW[kk * strideW + n] = (k < K && n < N) ? W[(size_t)n * K + k] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int kb = k0 + 4 * ks;
            if (4 * ks >= slab_rows || kb >= Kp) break;
            const int k = kb + lk;
            const float a = (k < K) ? arow[k] : 0.f;
            const float *bp = sW + (4 * ks + lk) * strideW + lrow;
#pragma unroll
            for (int j = 0; j < SMM_FLOW_JMAX; ++j)
                if (cg + j * ncg < NT) acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bp[(cg + j * ncg) * 16], acc[j], 0, 0, 0);
        }
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SMM_FLOW_JMAX; ++j) {
        const int nt = cg + j * ncg;
        if (nt >= NT) continue;
        const int n = nt * 16 + lrow;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = strip * 16 + lk * 4 + r;               // (C/D map of the 16x16 MFMAs: column on the lane)
            float *o = sOut + (size_t)row * strideOut + n;
            if (MODE == SMM_FLOW_RELU) *o = fmaxf(acc[j][r], 0.f);
            else if (MODE == SMM_FLOW_ADD) { if (n < N) *o = *o + acc[j][r]; }
            else *o = sMask[(size_t)row * strideMask + n] > 0.f ? acc[j][r] : 0.f;
        }
    }
}

// t_i(passive) of one coupling layer: activations a_1 .. a_{hl+1} into sA (one buffer, in place, or one per layer with `keep`),
// then the active half of sH += t (MODE ADD), or the activations alone (SKIP).  p: the layer's packed parameters.
template <int MODE>
__device__ __forceinline__ void smm_flow_couple(float *sH, int strideH, float *sA, int strideA, size_t act_step, float *sW,
                                                int strideW, const float *__restrict__ p, int i, int Dh, int H, int hl,
                                                int strips, int slab_rows)
{
    const int po = (i & 1) ? Dh : 0, ao = Dh - po;
    smm_flow_gemm<false, SMM_FLOW_RELU>(sH + po, strideH, Dh, sA, strideA, H, p, p + (size_t)Dh * H, nullptr, 0, sW, strideW,
                                        strips, slab_rows);
    p += (size_t)Dh * H + H;
    float *cur = sA;
#pragma nounroll
    for (int j = 0; j < hl; ++j) {
        smm_flow_gemm<false, SMM_FLOW_RELU>(cur, strideA, H, cur + act_step, strideA, H, p, p + (size_t)H * H, nullptr, 0, sW,
                                            strideW, strips, slab_rows);
        cur += act_step;
        p += (size_t)H * H + H;
    }
    if constexpr (MODE != SMM_FLOW_SKIP)
        smm_flow_gemm<false, MODE>(cur, strideA, H, sH + ao, strideH, Dh, p, p + (size_t)H * Dh, nullptr, 0, sW, strideW, strips,
                                   slab_rows);
}

// the active half (columns ao .. ao + Dh) of every row of the tile: sH -> save, or back
__device__ __forceinline__ void smm_flow_copy_half(float *dst, int strideDst, const float *src, int strideSrc, int M, int Dh)
{
    const int wave = smm_flow_wave(), lane = threadIdx.x & 63;
#pragma nounroll
    for (int r = wave; r < M; r += 4)
#pragma nounroll
        for (int c = lane; c < Dh; c += 64) dst[(size_t)r * strideDst + c] = src[(size_t)r * strideSrc + c];
}

__device__ __forceinline__ void smm_flow_load_tile(float *sT, int strideT, const float *__restrict__ src, int64_t row0,
                                                   int64_t n_rows, int M, int D)
{
    const int wave = smm_flow_wave(), lane = threadIdx.x & 63;
#pragma nounroll
    for (int r = wave; r < M; r += 4) {
        const bool live = row0 + r < n_rows;
        const float *s = src + (size_t)(row0 + (live ? r : 0)) * D;
#pragma nounroll
        for (int c = lane; c < D; c += 64) sT[(size_t)r * strideT + c] = live ? s[c] : 0.f;   // (rows past the end: zeros)
    }
}

__device__ __forceinline__ void smm_flow_store_tile(const float *sT, int strideT, float *__restrict__ dst, int64_t row0,
                                                    int64_t n_rows, int M, int D)
{
    const int wave = smm_flow_wave(), lane = threadIdx.x & 63;
#pragma nounroll
    for (int r = wave; r < M; r += 4) {
        if (row0 + r >= n_rows) break;
        float *o = dst + (size_t)(row0 + r) * D;
#pragma nounroll
        for (int c = lane; c < D; c += 64) o[c] = sT[(size_t)r * strideT + c];
    }
}

extern __shared__ __attribute__((aligned(16))) float smm_flow_lds[];

__global__ void __launch_bounds__(256) smm_flow_fwd_kernel(SmmFlowArgs a)
{
    const int D = a.d, Dh = D >> 1, H = a.h, hl = a.hidden_layers, M = 16 * a.strips;
    const int Hp = (H + 15) & ~15, Dp = (Dh + 15) & ~15;
    const int strideH = smm_flow_row_stride(D), strideA = smm_flow_row_stride(Hp), strideW = smm_flow_slab_stride(Hp > Dp ? Hp : Dp);
    float *sH = smm_flow_lds, *sA = sH + (size_t)M * strideH, *sW = sA + (size_t)M * strideA;
    const size_t per_layer = smm_flow_layer_params(Dh, H, hl);
#pragma nounroll
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t row0 = (int64_t)tile * M;
        __syncthreads();                                           // (the previous tile has been written out)
        smm_flow_load_tile(sH, strideH, a.x, row0, a.n_rows, M, D);
#pragma nounroll
        for (int i = 0; i < a.couple_layers; ++i)
            smm_flow_couple<SMM_FLOW_ADD>(sH, strideH, sA, strideA, 0, sW, strideW, a.params + i * per_layer, i, Dh, H, hl,
                                          a.strips, a.slab_rows);
        __syncthreads();
        smm_flow_store_tile(sH, strideH, a.out, row0, a.n_rows, M, D);
    }
}

// gW[k][n] += sum over the tile's rows of Act[row][k] Gz[row][n] (k < K, n < N): one MFMA chain over the rows per 16 x 16 block,
// the blocks dealt to the waves in a fixed order; gB[n] += sum over the rows of Gz[row][n].  Reads LDS, writes the partial.
__device__ __forceinline__ void smm_flow_param_grad(const float *sAct, int strideAct, int K, const float *sGz, int strideG, int N,
                                                    double *__restrict__ gW, double *__restrict__ gB, int M)
{
    const int tid = threadIdx.x, wave = smm_flow_wave(), lane = tid & 63, lcol = lane & 15, lk = lane >> 4;
    __syncthreads();
    const int KT = (K + 15) >> 4, NT = (N + 15) >> 4;
#pragma nounroll
    for (int p = wave; p < KT * NT; p += 4) {
        const int kt = p / NT, nt = p - kt * NT;
        const int kcol = kt * 16 + lcol, ncol = nt * 16 + lcol;
        smm_f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma nounroll
        for (int r0 = 0; r0 < M; r0 += 4) {
            const int r = r0 + lk;
            const float av = kcol < K ? sAct[(size_t)r * strideAct + kcol] : 0.f;     // A[i = k][row], B[row][j = n]
            const float bv = ncol < N ? sGz[(size_t)r * strideG + ncol] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int k = kt * 16 + lk * 4 + r;
            if (k < K && ncol < N) gW[(size_t)k * N + ncol] += (double)acc[r];
        }
    }
#pragma nounroll
    for (int n = tid; n < N; n += 256) {
        double s = 0.0;
#pragma nounroll
        for (int r = 0; r < M; ++r) s += (double)sGz[(size_t)r * strideG + n];
        gB[n] += s;
    }
}

__global__ void __launch_bounds__(256) smm_flow_bwd_kernel(SmmFlowArgs a)
{
    const int D = a.d, Dh = D >> 1, H = a.h, hl = a.hidden_layers, M = 16 * a.strips;
    const int Hp = (H + 15) & ~15, Dp = (Dh + 15) & ~15;
    const int strideH = smm_flow_row_stride(D), strideA = smm_flow_row_stride(Hp), strideW = smm_flow_slab_stride(Hp > Dp ? Hp : Dp);
    const size_t act = (size_t)M * strideA;
    float *sH = smm_flow_lds, *sG = sH + (size_t)M * strideH, *sA = sG + (size_t)M * strideH, *sW = sA + (size_t)(hl + 1) * act;
    // [couple_layers][M][Dh]: each layer's active half as it came in -- in LDS, or in this workgroup's slice of the scratch
    float *sKeep = a.keep == 1 ? sW + (size_t)a.slab_rows * strideW : a.keep_global + (size_t)blockIdx.x * a.couple_layers * M * Dh;
    const size_t keep_step = (size_t)M * Dh;
    const size_t per_layer = smm_flow_layer_params(Dh, H, hl);
    double *part = a.partials + (size_t)blockIdx.x * a.n_params;
#pragma nounroll
    for (int tile = blockIdx.x; tile < a.n_tiles; tile += gridDim.x) {
        const int64_t row0 = (int64_t)tile * M;
        __syncthreads();
        smm_flow_load_tile(sH, strideH, a.x, row0, a.n_rows, M, D);
        smm_flow_load_tile(sG, strideH, a.g_y, row0, a.n_rows, M, D);   // (rows past the end: zero gradient, they add nothing)
#pragma nounroll
        for (int i = 0; i < a.couple_layers; ++i) {
            __syncthreads();                                       // (the half was written by the load, or two layers ago)
            smm_flow_copy_half(sKeep + i * keep_step, Dh, sH + ((i & 1) ? 0 : Dh), strideH, M, Dh);
            smm_flow_couple<SMM_FLOW_ADD>(sH, strideH, sA, strideA, 0, sW, strideW, a.params + i * per_layer, i, Dh, H, hl,
                                          a.strips, a.slab_rows);
        }
#pragma nounroll
        for (int i = a.couple_layers - 1; i >= 0; --i) {
            const float *p = a.params + i * per_layer;
            double *g = part + i * per_layer;
            const int po = (i & 1) ? Dh : 0, ao = Dh - po;
            // sH: the layer's output -> its input; sA[j]: a_{j+1}
            // nothing of this layer's backward reads its active half; the layers below read it as it was, bit for bit
            // (copy_half deals the elements to the lanes the same way both times: a lane reads back what it wrote itself)
            smm_flow_couple<SMM_FLOW_SKIP>(sH, strideH, sA, strideA, act, sW, strideW, p, i, Dh, H, hl, a.strips, a.slab_rows);
            smm_flow_copy_half(sH + ao, strideH, sKeep + i * keep_step, Dh, M, Dh);
            // out_layer: dL/dz = the active half of sG; the gradient of a_{hl+1}, masked, replaces a_{hl+1}
            size_t off = (size_t)Dh * H + H + (size_t)hl * ((size_t)H * H + H);
            float *top = sA + (size_t)hl * act;
            smm_flow_param_grad(top, strideA, H, sG + ao, strideH, Dh, g + off, g + off + (size_t)H * Dh, M);
            smm_flow_gemm<true, SMM_FLOW_MASK>(sG + ao, strideH, Dh, top, strideA, H, p + off, nullptr, top, strideA, sW, strideW,
                                               a.strips, a.slab_rows);
            // hidden layers, last to first: dL/dz_{j+1} sits where a_{j+1} was
#pragma nounroll
            for (int j = hl; j >= 1; --j) {
                off -= (size_t)H * H + H;
                float *gz = sA + (size_t)j * act, *prev = sA + (size_t)(j - 1) * act;
                smm_flow_param_grad(prev, strideA, H, gz, strideA, H, g + off, g + off + (size_t)H * H, M);
                smm_flow_gemm<true, SMM_FLOW_MASK>(gz, strideA, H, prev, strideA, H, p + off, nullptr, prev, strideA, sW, strideW,
                                                   a.strips, a.slab_rows);
            }
            // in_layer: its input is the passive half, whose gradient takes the MLP's share on top of the copy's
            smm_flow_param_grad(sH + po, strideH, Dh, sA, strideA, H, g, g + (size_t)Dh * H, M);
            smm_flow_gemm<true, SMM_FLOW_ADD>(sA, strideA, H, sG + po, strideH, Dh, p, nullptr, nullptr, 0, sW, strideW, a.strips,
                                              a.slab_rows);
        }
        __syncthreads();
        if (a.out) smm_flow_store_tile(sG, strideH, a.out, row0, a.n_rows, M, D);
    }
}

__global__ void __launch_bounds__(256) smm_flow_reduce_kernel(const double *__restrict__ partials, int grid, size_t n_params,
                                                              double *__restrict__ g_params)
{
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_params; i += (size_t)gridDim.x * 256) {
        double s = 0.0;
        for (int g = 0; g < grid; ++g) s += partials[(size_t)g * n_params + i];
        g_params[i] = s;
    }
}

template <typename K>
static void smm_flow_raise_lds(K kernel, bool *raised)
{
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (!raised[dev]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, SMM_FLOW_LDS_MAX);
        raised[dev] = true;
    }
}

void smm_launch_flow_fwd(const SmmFlowArgs &a, const SmmFlowPlan &p, hipStream_t stream)
{
    static bool raised[64];
    smm_flow_raise_lds(smm_flow_fwd_kernel, raised);
    hipLaunchKernelGGL(smm_flow_fwd_kernel, dim3(p.grid), dim3(256), p.lds_bytes, stream, a);
}

void smm_launch_flow_bwd(const SmmFlowArgs &a, const SmmFlowPlan &p, hipStream_t stream)
{
    static bool raised[64];
    smm_flow_raise_lds(smm_flow_bwd_kernel, raised);
    hipLaunchKernelGGL(smm_flow_bwd_kernel, dim3(p.grid), dim3(256), p.lds_bytes, stream, a);
}

void smm_launch_flow_reduce(const double *partials, int grid, size_t n_params, double *g_params, hipStream_t stream)
{
    const int blocks = (int)std::min<size_t>((n_params + 255) / 256, 4096);
    hipLaunchKernelGGL(smm_flow_reduce_kernel, dim3(blocks), dim3(256), 0, stream, partials, grid, n_params, g_params);
}

// ------------------------------------------------------------------------------------------------ d elp / d x
// elp[t][c] = cst[g][c] + sum_d x[t][d] w[g][d][c] - 0.5 sum_d x[t][d]^2 inv_var[d]   ==>   with ge = dL/d elp:
//   g_x[t][d] = sum_c ge[t][c] w[g][d][c] - x[t][d] inv_var[d] sum_c ge[t][c]
// Thread = feature column, its row of w in registers (as smm_emission_bwd_kernel keeps its sums); the ge rows of a 64-frame
// tile and their sums sit in LDS and are read as broadcasts.  fp64 throughout, rounded once on the way out.
#define SMM_EBX_TILE 64

__device__ __forceinline__ int smm_ebx_find_video(const int32_t *__restrict__ cum, int n, int b)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (cum[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

template <int CT>
__global__ void __launch_bounds__(256) smm_emission_bwd_x_kernel(SmmEmBwdXArgs a)
{
    __shared__ __attribute__((aligned(16))) double s_ge[SMM_EBX_TILE * CT];
    __shared__ double s_rs[SMM_EBX_TILE];
    const int tid = threadIdx.x;
    const int D = a.d, cm = a.c_max;
    const int chunk = a.chunk;
    for (int it = blockIdx.x; it < a.n_chunks; it += gridDim.x) {
        const int slot = smm_ebx_find_video(a.cum, a.b, it);
        const SmmVideo mv = a.videos[a.order[slot]];
        const int g = mv.group, C = min(a.n_states[g], CT);
        const int r0 = (it - a.cum[slot]) * chunk, r1 = min(mv.T, r0 + chunk);
        for (int c0 = 0; c0 < D; c0 += 256) {
            const int col = c0 + tid;
            const bool real = col < D;
            const int colc = real ? col : 0;                       // (idle lanes work on column 0 and drop the result)
            double wr[CT];
            const double *__restrict__ wp = a.w + ((size_t)g * D + colc) * cm;
#pragma unroll
            for (int c = 0; c < CT; ++c) wr[c] = c < C ? wp[c] : 0.0;
            const double iv = a.inv_var[colc];
            for (int t0 = r0; t0 < r1; t0 += SMM_EBX_TILE) {
                const int nt = min(SMM_EBX_TILE, r1 - t0);
                const double *__restrict__ ge = a.g_elp + (size_t)(mv.frame_off + t0) * cm;
                __syncthreads();                                   // the previous tile has been consumed
                for (int i = tid; i < SMM_EBX_TILE * CT; i += 256) {
                    const int f = i / CT, c = i - f * CT;
                    s_ge[i] = (f < nt && c < C) ? ge[(size_t)f * cm + c] : 0.0;
                }
                __syncthreads();
                if (tid < SMM_EBX_TILE) {
                    double r = 0.0;
#pragma unroll
                    for (int c = 0; c < CT; ++c) r += s_ge[tid * CT + c];
                    s_rs[tid] = r;
                }
                __syncthreads();
                const float *__restrict__ xp = a.x + (size_t)(mv.frame_off + t0) * D + colc;
                float *__restrict__ op = a.g_x + (size_t)(mv.frame_off + t0) * D + colc;
                for (int f = 0; f < nt; ++f) {
                    const double *gr = s_ge + f * CT;
                    double s = 0.0;
#pragma unroll
                    for (int c = 0; c < CT; ++c) s = __builtin_fma(gr[c], wr[c], s);
                    const double v = s - (double)xp[(size_t)f * D] * iv * s_rs[f];
                    if (real) op[(size_t)f * D] = (float)v;
                }
            }
        }
    }
}

void smm_launch_emission_bwd_x(const SmmEmBwdXArgs &a, int c_need, hipStream_t stream)
{
    const int grid = a.n_chunks < 65536 ? a.n_chunks : 65536;
    if (c_need <= 8) hipLaunchKernelGGL(smm_emission_bwd_x_kernel<8>, dim3(grid), dim3(256), 0, stream, a);
    else if (c_need <= 16) hipLaunchKernelGGL(smm_emission_bwd_x_kernel<16>, dim3(grid), dim3(256), 0, stream, a);
    else if (c_need <= 24) hipLaunchKernelGGL(smm_emission_bwd_x_kernel<24>, dim3(grid), dim3(256), 0, stream, a);
    else hipLaunchKernelGGL(smm_emission_bwd_x_kernel<32>, dim3(grid), dim3(256), 0, stream, a);
}
