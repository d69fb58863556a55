// featnet.hip -- the ResUNetSmall2 forward pass (reference models.py:392-618, configuration :691-698) on gather-GEMM sparse
// convolution, and the C ABI of include/umereg_featnet.h.
//
// Every 27-offset layer is one launch of fn_conv_kernel: output-stationary, a tile of TM output rows x TN output channels per
// workgroup, f32 MFMA (v_mfma_f32_32x32x2_f32) over the offsets the tile's rows use (the OR of their neighbour masks) and 32-
// channel slices of C_in, the gathered input rows staged in LDS (a missing neighbour stages zeros).  Every output element is one
// fixed chain -- offsets ascending, channels ascending -- whatever the tile or the row order: bit-identical run to run, no
// atomics.  The epilogue applies the folded eval batch norm (scale, shift), the block's residual and ReLU, and writes at a
// column offset of a wider row, so ME.cat(tr, skip) is where the two producers write: no copy.  conv1 (C_in = 1) and the
// `final` 1x1 layer with its L2 normalisation have their own small kernels; mlp1 is the generic kernel with K = 1.
//
// The single-layer entries of include/umereg_sparse_conv.h that launch these kernels live here too (a kernel is launched only
// from the unit that defines it): the plain convolution over one table (fn_conv_kernel with the caller's scale / shift block,
// no ReLU, the residual input used only to accumulate channel slices into the output) and conv1's forward.  The training path's own kernels are in sparse_wgrad.hip.
//
// The f16-operand inference mode (include/umereg_featnet_f16.h) is fn_conv_f16_kernel, the twin of fn_conv_kernel on
// v_mfma_f32_32x32x16_f16, launched for layers 1..18 by the same forward; conv1 and `final` are the f32 kernels in both modes.
//
// The entries of include/umereg_sparse_conv_pairs.h are the same two host paths (fn_forward, fn_sparse_conv) with `pairs` set:
// fn_launch_conv then hands every 27-offset layer to sparse_conv_pairs.hip, and keeps the 1x1 layers here.
#include <math.h>

#include "sparse.h"
#include "umereg_featnet_f16.h"
#include "umereg_sparse_conv.h"
#include "umereg_sparse_conv_pairs.h"

namespace umereg {

namespace {

struct FnLayer {
    int K, cin, cout;
};
// layer order of the packed parameter block (python: models.LAYERS names them)
constexpr FnLayer kFnLayers[UMEREG_FEATNET_LAYERS] = {
    {27, 1, 32},    {27, 32, 32},   {27, 32, 64},   {27, 64, 64},   {27, 64, 64},   {27, 64, 64},   {27, 64, 128},
    {27, 128, 128}, {27, 128, 256}, {27, 256, 256}, {27, 256, 128}, {27, 128, 128}, {27, 256, 128}, {27, 128, 128},
    {27, 192, 64},  {27, 64, 64},   {27, 128, 64},  {27, 64, 64},   {1, 96, 64},    {1, 64, 32}};

struct FnParamOffsets {
    size_t w[UMEREG_FEATNET_LAYERS], scale[UMEREG_FEATNET_LAYERS], total;
};

FnParamOffsets fn_params()
{
    FnParamOffsets p;
    size_t o = 0;
    for (int i = 0; i < UMEREG_FEATNET_LAYERS; ++i) {
        const FnLayer& L = kFnLayers[i];
        p.w[i] = o;
        o = align_up(o + (size_t)L.K * L.cin * L.cout, 4);
        p.scale[i] = o;
        o = align_up(o + 2 * (size_t)L.cout, 4);
    }
    p.total = o;
    return p;
}

typedef float f32x16 __attribute__((ext_vector_type(16)));
constexpr int kKC = 32;     // input channels per staged slice

template <int TM, int TN>
__global__ __launch_bounds__(256) void fn_conv_kernel(ConvArgs a)
{
    constexpr int WM = TM / 32;                 // waves along the rows; (TM / 32) x (TN / 32) = 4 waves
    constexpr int TPR = 256 / TM;               // staging threads per input row
    constexpr int AF = kKC / TPR;               // floats each of them stages
    constexpr int BF = kKC * TN / 256;          // weight floats per thread
    constexpr int BTPR = TN / BF;
    static_assert(WM * (TN / 32) == 4 && AF % 4 == 0 && BF % 4 == 0 && 256 / BTPR == kKC, "tile shape");
    __shared__ float As[TM][kKC + 1];
    __shared__ __attribute__((aligned(16))) float Bs[kKC][TN];
    __shared__ int Ns[TM][kFnVol];              // the tile's neighbour rows
    __shared__ unsigned int s_mask;

    const int n_rows = *a.n_out;
    const int m0 = blockIdx.x * TM;
    if (m0 >= n_rows) return;
    const int n0 = blockIdx.y * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    if (tid == 0) s_mask = a.K > 1 ? 0u : 1u;
    if (a.K > 1) {
        const int* nb = a.nbr + (size_t)m0 * kFnVol;
        for (int e = tid; e < TM * kFnVol; e += 256) Ns[e / kFnVol][e % kFnVol] = m0 + e / kFnVol < n_rows ? nb[e] : -1;
    }
    __syncthreads();
    if (a.K > 1 && tid < TM && m0 + tid < n_rows) atomicOr(&s_mask, a.mask[m0 + tid]);
    __syncthreads();

    // steps: (offset k, channel slice) over the offsets some row of the tile uses, k ascending; the global loads of step s + 1
    // are in flight while the MFMAs of step s run
    const int lr = tid / TPR, seg = tid % TPR, arow = m0 + lr;
    const int br = tid / BTPR, bc = (tid % BTPR) * BF;
    const int n_sl = a.cin / kKC;
    unsigned int rem = s_mask;
    int k = rem ? __builtin_ctz(rem) : 0, sl = 0;
    float4 av[AF / 4], bv[BF / 4];
    auto load = [&](int k_, int sl_) {
        const int src = arow < n_rows ? (a.K > 1 ? Ns[lr][k_] : arow) : -1;
        if (src >= 0) {
            const float4* p = reinterpret_cast<const float4*>(a.in + (size_t)src * a.ld_in + sl_ * kKC + seg * AF);
#pragma unroll
            for (int j = 0; j < AF / 4; ++j) av[j] = p[j];
        } else {
#pragma unroll
            for (int j = 0; j < AF / 4; ++j) av[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float4* q = reinterpret_cast<const float4*>(a.W + ((size_t)k_ * a.cin + sl_ * kKC + br) * a.cout + n0 + bc);
#pragma unroll
        for (int j = 0; j < BF / 4; ++j) bv[j] = q[j];
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (rem) load(k, sl);
    while (rem) {
        __syncthreads();                              // the previous step's LDS tiles are consumed
#pragma unroll
        for (int j = 0; j < AF / 4; ++j) {
            As[lr][seg * AF + 4 * j + 0] = av[j].x;
            As[lr][seg * AF + 4 * j + 1] = av[j].y;
            As[lr][seg * AF + 4 * j + 2] = av[j].z;
            As[lr][seg * AF + 4 * j + 3] = av[j].w;
        }
#pragma unroll
        for (int j = 0; j < BF / 4; ++j) *reinterpret_cast<float4*>(&Bs[br][bc + 4 * j]) = bv[j];
        __syncthreads();
        if (++sl == n_sl) {
            sl = 0;
            rem &= rem - 1u;
            k = rem ? __builtin_ctz(rem) : 0;
        }
        if (rem) load(k, sl);
        // lane l: A[row l & 31][k = l >> 5], B[k = l >> 5][col l & 31]
#pragma unroll
        for (int kk = 0; kk < kKC / 2; ++kk) {
            const float x = As[wm * 32 + (lane & 31)][2 * kk + (lane >> 5)];
            const float y = Bs[2 * kk + (lane >> 5)][wn * 32 + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, acc, 0, 0, 0);
        }
    }
    // C/D: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int col = n0 + wn * 32 + (lane & 31);
    const float sc = a.scale[col], sh = a.shift[col];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= n_rows) continue;
        float v = fmaf(acc[r], sc, sh);
        if (a.res) v += a.res[(size_t)row * a.ld_res + col];
        if (a.relu) v = fmaxf(v, 0.f);
        a.out[(size_t)row * a.ld_out + col] = v;
    }
}

// conv1 + norm1: C_in = 1, 32 outputs; the input feature of level-0 row j is feat[perm[j]]
__global__ __launch_bounds__(256) void fn_conv1_kernel(const float* __restrict__ feat, const int* __restrict__ perm, const int* __restrict__ nbr,
                                                       const int32_t* __restrict__ n_out, const float* __restrict__ W,
                                                       const float* __restrict__ scale, const float* __restrict__ shift, float* __restrict__ out)
{
    const int row = blockIdx.x * 8 + (threadIdx.x >> 5), c = threadIdx.x & 31;
    if (row >= *n_out) return;
    float acc = 0.f;
    for (int k = 0; k < kFnVol; ++k) {
        const int j = nbr[(size_t)row * kFnVol + k];
        if (j >= 0) acc = fmaf(feat[perm[j]], W[k * 32 + c], acc);
    }
    out[(size_t)row * 32 + c] = fmaf(acc, scale[c], shift[c]);
}

// final (64 -> 32, bias) + row-wise L2 normalisation, written at the row's input position
__global__ __launch_bounds__(256) void fn_final_kernel(const float* __restrict__ h, const int* __restrict__ perm, const int32_t* __restrict__ n_out,
                                                       const float* __restrict__ W, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, float* __restrict__ out)
{
    __shared__ float Ws[64 * 32];
    for (int i = threadIdx.x; i < 64 * 32; i += 256) Ws[i] = W[i];
    __syncthreads();
    const int row = blockIdx.x * 256 + threadIdx.x;
    if (row >= *n_out) return;
    float acc[32];
#pragma unroll
    for (int c = 0; c < 32; ++c) acc[c] = 0.f;
    const float4* hr = reinterpret_cast<const float4*>(h + (size_t)row * 64);
    for (int i4 = 0; i4 < 16; ++i4) {
        const float4 v = hr[i4];
        const float hv[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int c = 0; c < 32; ++c) acc[c] = fmaf(hv[j], Ws[(4 * i4 + j) * 32 + c], acc[c]);
    }
    float ss = 0.f;
#pragma unroll
    for (int c = 0; c < 32; ++c) {
        acc[c] = fmaf(acc[c], scale[c], shift[c]);
        ss = fmaf(acc[c], acc[c], ss);
    }
    const float nrm = sqrtf(ss);
    float4* o = reinterpret_cast<float4*>(out + (size_t)perm[row] * 32);
#pragma unroll
    for (int c4 = 0; c4 < 8; ++c4)
        o[c4] = make_float4(acc[4 * c4] / nrm, acc[4 * c4 + 1] / nrm, acc[4 * c4 + 2] / nrm, acc[4 * c4 + 3] / nrm);
}

// ---- the f16-operand twin of fn_conv_kernel (include/umereg_featnet_f16.h) ------------------------------------------------------
//
// Same tiles, same offset walk, same prefetch and the same epilogue; the two staged tiles hold f16 (each gathered activation and
// each weight rounded to nearest even where the tile is staged) and a 32-channel step is two v_mfma_f32_32x32x16_f16 with f32
// accumulation: every output element is one fixed chain -- offsets ascending, channels ascending in groups of 16.
// For 32x32x16, lane l (r = l & 31, h = l >> 5) holds A[r][8h + j] and B[8h + j][r], j = 0..7: the A tile is [row][channel], the B
// tile is stored transposed, [output column][channel], so both fragments are 8 consecutive f16 = one 16-byte read.  Rows of 32
// f16 are padded by one read width (8 f16) to 80 bytes: the 16 lanes that ds_read_b128 serves in one cycle read 16 rows distinct
// mod 16, and 5 r mod 16 puts those on the 16 different 16-byte slots of the 256-byte bank row.
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr int kKP = kKC + 8;            // f16 per padded LDS row
constexpr float kF16Max = 65504.f;

template <int TM, int TN>
__global__ __launch_bounds__(256) void fn_conv_f16_kernel(ConvArgsF16 args)
{
    constexpr int WM = TM / 32;                 // waves along the rows; (TM / 32) x (TN / 32) = 4 waves
    constexpr int TPR = 256 / TM;               // staging threads per input row
    constexpr int AF = kKC / TPR;               // activations each of them stages
    constexpr int BF = kKC * TN / 256;          // weights per thread: BF consecutive channels of one output column
    static_assert(WM * (TN / 32) == 4 && AF % 8 == 0 && (BF == 4 || BF == 8) && (256 / TN) * BF == kKC, "tile shape");
    __shared__ __attribute__((aligned(16))) _Float16 As[TM][kKP];
    __shared__ __attribute__((aligned(16))) _Float16 Bt[TN][kKP];   // Bt[col][channel]
    __shared__ int Ns[TM][kFnVol];              // the tile's neighbour rows
    __shared__ unsigned int s_mask;

    const ConvArgs& a = args.c;
    const int n_rows = *a.n_out;
    const int m0 = blockIdx.x * TM;
    if (m0 >= n_rows) return;
    const int n0 = blockIdx.y * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    if (tid == 0) s_mask = a.K > 1 ? 0u : 1u;
    if (a.K > 1) {
        const int* nb = a.nbr + (size_t)m0 * kFnVol;
        for (int e = tid; e < TM * kFnVol; e += 256) Ns[e / kFnVol][e % kFnVol] = m0 + e / kFnVol < n_rows ? nb[e] : -1;
    }
    __syncthreads();
    if (a.K > 1 && tid < TM && m0 + tid < n_rows) atomicOr(&s_mask, a.mask[m0 + tid]);
    __syncthreads();

    // steps: (offset k, channel slice) over the offsets some row of the tile uses, k ascending; the global loads of step s + 1
    // (f32, as stored) are in flight while the MFMAs of step s run, and are rounded when they are staged
    const int lr = tid / TPR, seg = tid % TPR, arow = m0 + lr;
    const int bcol = tid % TN, bk = (tid / TN) * BF;
    const int n_sl = a.cin / kKC;
    unsigned int rem = s_mask;
    int k = rem ? __builtin_ctz(rem) : 0, sl = 0;
    float4 av[AF / 4];
    float bv[BF];
    auto load = [&](int k_, int sl_) {
        const int src = arow < n_rows ? (a.K > 1 ? Ns[lr][k_] : arow) : -1;
        if (src >= 0) {
            const float4* p = reinterpret_cast<const float4*>(a.in + (size_t)src * a.ld_in + sl_ * kKC + seg * AF);
#pragma unroll
            for (int j = 0; j < AF / 4; ++j) av[j] = p[j];
        } else {
#pragma unroll
            for (int j = 0; j < AF / 4; ++j) av[j] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        const float* q = a.W + ((size_t)k_ * a.cin + sl_ * kKC + bk) * a.cout + n0 + bcol;
#pragma unroll
        for (int j = 0; j < BF; ++j) bv[j] = q[(size_t)j * a.cout];
    };
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    if (rem) load(k, sl);
    while (rem) {
        __syncthreads();                              // the previous step's LDS tiles are consumed
#pragma unroll
        for (int j = 0; j < AF / 8; ++j) {
            f16x8 h;
            h[0] = (_Float16)av[2 * j].x, h[1] = (_Float16)av[2 * j].y, h[2] = (_Float16)av[2 * j].z, h[3] = (_Float16)av[2 * j].w;
            h[4] = (_Float16)av[2 * j + 1].x, h[5] = (_Float16)av[2 * j + 1].y, h[6] = (_Float16)av[2 * j + 1].z,
            h[7] = (_Float16)av[2 * j + 1].w;
            *reinterpret_cast<f16x8*>(&As[lr][seg * AF + 8 * j]) = h;
        }
#pragma unroll
        for (int j = 0; j < BF; ++j) Bt[bcol][bk + j] = (_Float16)bv[j];
        __syncthreads();
        if (++sl == n_sl) {
            sl = 0;
            rem &= rem - 1u;
            k = rem ? __builtin_ctz(rem) : 0;
        }
        if (rem) load(k, sl);
#pragma unroll
        for (int kk = 0; kk < kKC / 16; ++kk) {
            const f16x8 x = *reinterpret_cast<const f16x8*>(&As[wm * 32 + (lane & 31)][16 * kk + 8 * (lane >> 5)]);
            const f16x8 y = *reinterpret_cast<const f16x8*>(&Bt[wn * 32 + (lane & 31)][16 * kk + 8 * (lane >> 5)]);
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, acc, 0, 0, 0);
        }
    }
    // C/D: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int col = n0 + wn * 32 + (lane & 31);
    const float sc = a.scale[col], sh = a.shift[col];
    bool out_of_range = false;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        if (row >= n_rows) continue;
        float v = fmaf(acc[r], sc, sh);
        if (a.res) v += a.res[(size_t)row * a.ld_res + col];
        out_of_range |= v != v;                       // (a NaN, which the ReLU would hide, comes from infinities met on the way)
        if (a.relu) v = fmaxf(v, 0.f);
        out_of_range |= fabsf(v) > kF16Max;
        a.out[(size_t)row * a.ld_out + col] = v;
    }
    if (args.range && out_of_range) atomicOr(args.range, UMEREG_FN_ERR_F16_RANGE);
}

// one convolution launch over at most `rows_bound` output rows: 64 x 64 tiles where C_out allows, else 128 x 32; `range` as ConvArgsF16.
// `pairs`: a 27-offset layer goes to the pair-compacted engine of sparse_conv_pairs.hip instead (a 1x1 layer has every row active and
// stays here)
int fn_launch_conv(const ConvArgs& a, bool f16, int32_t* range, int rows_bound, hipStream_t st, bool pairs = false)
{
    if (pairs && a.K > 1) return fn_launch_conv_pairs(a, f16, range, rows_bound, st);
    const bool wide = a.cout % 64 == 0;
    const dim3 grid = wide ? dim3((rows_bound + 63) / 64, a.cout / 64) : dim3((rows_bound + 127) / 128, a.cout / 32);
    const ConvArgsF16 h{a, range};
    if (f16 && wide) hipLaunchKernelGGL((fn_conv_f16_kernel<64, 64>), grid, dim3(256), 0, st, h);
    else if (f16) hipLaunchKernelGGL((fn_conv_f16_kernel<128, 32>), grid, dim3(256), 0, st, h);
    else if (wide) hipLaunchKernelGGL((fn_conv_kernel<64, 64>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((fn_conv_kernel<128, 32>), grid, dim3(256), 0, st, a);
    UMEREG_CHECK_LAUNCH(f16 ? "fn_conv_f16_kernel" : "fn_conv_kernel");
    return UMEREG_OK;
}

struct Fwd {
    const float* params;
    FnParamOffsets po;
    char* ws;
    FnWs w;
    int32_t* status;
    hipStream_t st;
    bool f16;               // layers 1..18 on fn_conv_f16_kernel
    bool pairs;             // layers 1..17 on the pair-compacted engine (include/umereg_sparse_conv_pairs.h)

    float* buf(size_t off) const { return reinterpret_cast<float*>(ws + off); }

    // layer `i` over map `m` (-1: 1x1): in (ld_in) -> out (ld_out), optional residual
    int conv(int i, int m, const float* in, int ld_in, float* out, int ld_out, const float* res, int ld_res, bool relu) const
    {
        const FnLayer& L = kFnLayers[i];
        const FnTable t = fn_table(ws, w, m);
        ConvArgs a;
        a.in = in, a.W = params + po.w[i], a.scale = params + po.scale[i], a.shift = params + po.scale[i] + L.cout;
        a.res = res, a.out = out, a.nbr = t.nbr, a.mask = t.mask, a.n_out = status + 1 + t.level;
        a.ld_in = ld_in, a.ld_res = ld_res, a.ld_out = ld_out, a.cin = L.cin, a.cout = L.cout, a.K = L.K, a.relu = relu ? 1 : 0;
        // the range check covers what a later f16 layer gathers: mlp1's output feeds `final`, which is f32
        return fn_launch_conv(a, f16, i < 18 ? status : nullptr, w.n, st, pairs);
    }
};

}  // namespace

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_featnet_params_count(void) { return fn_params().total; }

UMEREG_API int umereg_featnet_layer_info(int layer, int32_t* info)
{
    UMEREG_REQUIRE(info, "featnet_layer_info: null pointer");
    UMEREG_REQUIRE(layer >= 0 && layer < UMEREG_FEATNET_LAYERS, "featnet_layer_info: layer %d out of range", layer);
    const FnParamOffsets p = fn_params();
    const FnLayer& L = kFnLayers[layer];
    info[0] = L.K, info[1] = L.cin, info[2] = L.cout, info[3] = (int32_t)p.w[layer], info[4] = (int32_t)p.scale[layer];
    return UMEREG_OK;
}

UMEREG_API size_t umereg_featnet_workspace_bytes(int n, int batch)
{
    if (n <= 0 || batch <= 0 || batch > UMEREG_FEATNET_MAX_BATCH) return 0;
    return fn_ws(n).total;
}

UMEREG_API int umereg_featnet_buffer(int n, int batch, int which, size_t* offset, int32_t* cols)
{
    UMEREG_REQUIRE(offset && cols, "featnet_buffer: null pointer");
    UMEREG_REQUIRE(n > 0 && batch > 0 && batch <= UMEREG_FEATNET_MAX_BATCH, "featnet_buffer: bad n %d / batch %d", n, batch);
    UMEREG_REQUIRE(which >= 0 && which < UMEREG_FN_NBUF, "featnet_buffer: buffer %d out of range", which);
    const FnWs w = fn_ws(n);
    if (which < UMEREG_FN_CAT0) {
        *offset = w.off_coords + (size_t)(which - UMEREG_FN_COORDS0) * n * 16, *cols = 4;
    } else if (which < UMEREG_FN_S4) {
        *offset = w.off_cat[which - UMEREG_FN_CAT0], *cols = kFnCatCols[which - UMEREG_FN_CAT0];
    } else if (which == UMEREG_FN_S4) {
        *offset = w.off_s4, *cols = 256;
    } else if (which == UMEREG_FN_HIDDEN) {
        *offset = w.off_x, *cols = 64;
    } else if (which == UMEREG_FN_PERM) {
        *offset = w.off_perm, *cols = 1;
    } else {
        *offset = w.off_mask, *cols = kFnMaps;      // (as [13][n]: n rows of 13 words in total)
    }
    return UMEREG_OK;
}

namespace {
int fn_check_maps_args(const int32_t* coords, int n, int batch, const int32_t* status, const void* workspace, size_t workspace_bytes)
{
    UMEREG_REQUIRE(coords && status, "featnet: null pointer");
    UMEREG_REQUIRE(n > 0, "featnet: n must be positive (got %d)", n);
    UMEREG_REQUIRE(batch > 0 && batch <= UMEREG_FEATNET_MAX_BATCH, "featnet: batch %d outside [1, %d]", batch, UMEREG_FEATNET_MAX_BATCH);
    UMEREG_REQUIRE(((uintptr_t)coords & 15) == 0, "featnet: coords must be 16-byte aligned");
    if (int rc = check_device()) return rc;
    return fn_check_ws("featnet", workspace, workspace_bytes, n);
}
}  // namespace

UMEREG_API int umereg_featnet_build_maps(const int32_t* coords, int n, int batch, int32_t* status, void* workspace, size_t workspace_bytes,
                                         void* stream)
{
    if (int rc = fn_check_maps_args(coords, n, batch, status, workspace, workspace_bytes)) return rc;
    return fn_build_maps(coords, n, batch, (char*)workspace, status, (hipStream_t)stream);
}

namespace {
// the forward pass of both precisions (f16: layers 1..18 on fn_conv_f16_kernel; conv1 and `final` are the f32 kernels either way)
int fn_forward(const int32_t* coords, const float* feat, int n, int batch, const float* params, float* out, int32_t* status,
               void* workspace, size_t workspace_bytes, void* stream, bool f16, bool pairs = false)
{
    UMEREG_REQUIRE(feat && params && out, "featnet_forward: null pointer");
    UMEREG_REQUIRE(((uintptr_t)params & 15) == 0 && ((uintptr_t)out & 15) == 0, "featnet_forward: params and out must be 16-byte aligned");
    if (int rc = fn_check_maps_args(coords, n, batch, status, workspace, workspace_bytes)) return rc;
    const FnWs w = fn_ws(n);
    hipStream_t st = (hipStream_t)stream;
    char* ws = (char*)workspace;
    if (int rc = fn_build_maps(coords, n, batch, ws, status, st)) return rc;

    Fwd f{params, fn_params(), ws, w, status, st, f16, pairs};
    float* X = f.buf(w.off_x);
    float* S4 = f.buf(w.off_s4);
    float* cat[4];
    for (int l = 0; l < 4; ++l) cat[l] = f.buf(w.off_cat[l]);
    const int* perm = reinterpret_cast<const int*>(ws + w.off_perm);

    // encoder: conv -> BN (X), block -> the skip columns of the level's concatenation (level 4: S4)
    hipLaunchKernelGGL(fn_conv1_kernel, dim3((n + 7) / 8), dim3(256), 0, st, feat, perm, fn_table(ws, w, fn_map_self(0)).nbr, status + 1,
                       params + f.po.w[0], params + f.po.scale[0], params + f.po.scale[0] + 32, X);
    UMEREG_CHECK_LAUNCH("fn_conv1_kernel");
    int rc = f.conv(1, fn_map_self(0), X, 32, cat[0] + kFnCatTr[0], kFnCatCols[0], X, 32, true);
    for (int l = 1; l < kFnLevels && !rc; ++l) {
        const int cout = kFnLayers[2 * l].cout;
        rc = f.conv(2 * l, fn_map_down(l - 1), cat[l - 1] + kFnCatTr[l - 1], kFnCatCols[l - 1], X, cout, nullptr, 0, false);
        float* dst = l < 4 ? cat[l] + kFnCatTr[l] : S4;
        const int ld = l < 4 ? kFnCatCols[l] : 256;
        if (!rc) rc = f.conv(2 * l + 1, fn_map_self(l), X, cout, dst, ld, X, cout, true);
    }
    // decoder: transposed conv -> BN (X), block -> the first columns of the finer level's concatenation
    for (int l = 3; l >= 0 && !rc; --l) {
        const int i = 10 + 2 * (3 - l);
        const int cout = kFnLayers[i].cout;
        const float* src = l == 3 ? S4 : cat[l + 1];
        const int ld_src = l == 3 ? 256 : kFnCatCols[l + 1];
        rc = f.conv(i, fn_map_up(l), src, ld_src, X, cout, nullptr, 0, false);
        if (!rc) rc = f.conv(i + 1, fn_map_self(l), X, cout, cat[l], kFnCatCols[l], X, cout, true);
    }
    // mlp1 + ReLU -> X [n, 64]; final + L2 normalisation -> out in input row order
    if (!rc) rc = f.conv(18, -1, cat[0], kFnCatCols[0], X, 64, nullptr, 0, true);
    if (rc) return rc;
    hipLaunchKernelGGL(fn_final_kernel, dim3((n + 255) / 256), dim3(256), 0, st, X, perm, status + 1, params + f.po.w[19],
                       params + f.po.scale[19], params + f.po.scale[19] + 32, out);
    UMEREG_CHECK_LAUNCH("fn_final_kernel");
    return UMEREG_OK;
}
}  // namespace

UMEREG_API int umereg_featnet_forward_f32(const int32_t* coords, const float* feat, int n, int batch, const float* params, float* out,
                                          int32_t* status, void* workspace, size_t workspace_bytes, void* stream)
{
    return fn_forward(coords, feat, n, batch, params, out, status, workspace, workspace_bytes, stream, false);
}

// ---- include/umereg_featnet_f16.h ---------------------------------------------------------------------------------------------

UMEREG_API int umereg_featnet_forward_f16(const int32_t* coords, const float* feat, int n, int batch, const float* params, float* out,
                                          int32_t* status, void* workspace, size_t workspace_bytes, void* stream)
{
    return fn_forward(coords, feat, n, batch, params, out, status, workspace, workspace_bytes, stream, true);
}

// ---- include/umereg_sparse_conv.h: the entries that launch this unit's kernels ---------------------------------------------------

namespace {
// the plain convolution of both precisions; f16 also takes table -1: the 1x1 layer over level 0 (W [C_in][C_out])
int fn_sparse_conv(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, int table, const float* in, int ld_in,
                   const float* W, int c_in, int c_out, const float* scale, const float* shift, float* out, int ld_out, int accumulate,
                   void* stream, bool f16, bool pairs = false)
{
    UMEREG_REQUIRE(workspace && status && in && W && scale && shift && out, "sparse_conv: null pointer");
    UMEREG_REQUIRE(n > 0, "sparse_conv: n must be positive (got %d)", n);
    UMEREG_REQUIRE(table >= (f16 ? -1 : 0) && table < UMEREG_SPARSE_CONV_TABLES, "sparse_conv: table %d outside [%d, %d)", table,
                   f16 ? -1 : 0, UMEREG_SPARSE_CONV_TABLES);
    UMEREG_REQUIRE(c_in > 0 && c_in % 32 == 0 && c_in <= UMEREG_SPARSE_CONV_MAX_CH && c_out > 0 && c_out % 32 == 0 &&
                       c_out <= UMEREG_SPARSE_CONV_MAX_CH,
                   "sparse_conv: channels %d -> %d must be multiples of 32 up to %d", c_in, c_out, UMEREG_SPARSE_CONV_MAX_CH);
    UMEREG_REQUIRE(ld_in >= c_in && ld_in % 4 == 0 && ld_out >= c_out, "sparse_conv: bad leading dimensions %d / %d", ld_in, ld_out);
    UMEREG_REQUIRE(((uintptr_t)in & 15) == 0 && ((uintptr_t)W & 15) == 0, "sparse_conv: in and W must be 16-byte aligned");
    if (int rc = check_device()) return rc;
    if (int rc = fn_check_ws("sparse_conv", workspace, workspace_bytes, n)) return rc;
    const FnTable t = fn_table(workspace, fn_ws(n), table);
    ConvArgs a;
    a.in = in, a.W = W, a.scale = scale, a.shift = shift, a.res = accumulate ? out : nullptr, a.out = out;   // (res == out: each
                                                                                                             // element is read, then written, by one thread)
    a.nbr = t.nbr, a.mask = t.mask, a.n_out = status + 1 + t.level;
    a.ld_in = ld_in, a.ld_res = ld_out, a.ld_out = ld_out, a.cin = c_in, a.cout = c_out, a.K = table >= 0 ? kFnVol : 1, a.relu = 0;
    return fn_launch_conv(a, f16, nullptr, n, (hipStream_t)stream, pairs);
}
}  // namespace

UMEREG_API int umereg_sparse_conv_f32(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, int table,
                                      const float* in, int ld_in, const float* W, int c_in, int c_out, const float* scale,
                                      const float* shift, float* out, int ld_out, int accumulate, void* stream)
{
    return fn_sparse_conv(workspace, workspace_bytes, status, n, table, in, ld_in, W, c_in, c_out, scale, shift, out, ld_out, accumulate,
                          stream, false);
}

UMEREG_API int umereg_sparse_conv_f16(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, int table,
                                      const float* in, int ld_in, const float* W, int c_in, int c_out, const float* scale,
                                      const float* shift, float* out, int ld_out, int accumulate, void* stream)
{
    return fn_sparse_conv(workspace, workspace_bytes, status, n, table, in, ld_in, W, c_in, c_out, scale, shift, out, ld_out, accumulate,
                          stream, true);
}

// ---- include/umereg_sparse_conv_pairs.h: the same two host paths with the 27-offset layers on sparse_conv_pairs.hip -----------------

UMEREG_API int umereg_featnet_forward_pairs(const int32_t* coords, const float* feat, int n, int batch, const float* params, float* out,
                                            int32_t* status, void* workspace, size_t workspace_bytes, void* stream, int f16)
{
    return fn_forward(coords, feat, n, batch, params, out, status, workspace, workspace_bytes, stream, f16 != 0, true);
}

UMEREG_API int umereg_sparse_conv_pairs(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, int table,
                                        const float* in, int ld_in, const float* W, int c_in, int c_out, const float* scale,
                                        const float* shift, float* out, int ld_out, int accumulate, void* stream, int f16)
{
    return fn_sparse_conv(workspace, workspace_bytes, status, n, table, in, ld_in, W, c_in, c_out, scale, shift, out, ld_out, accumulate,
                          stream, f16 != 0, true);
}

UMEREG_API int umereg_sparse_conv1_f32(const void* workspace, size_t workspace_bytes, const int32_t* status, int n, const float* feat,
                                       const float* W, const float* scale, const float* shift, float* out, void* stream)
{
    UMEREG_REQUIRE(workspace && status && feat && W && scale && shift && out, "sparse_conv1: null pointer");
    UMEREG_REQUIRE(n > 0, "sparse_conv1: n must be positive (got %d)", n);
    if (int rc = check_device()) return rc;
    if (int rc = fn_check_ws("sparse_conv1", workspace, workspace_bytes, n)) return rc;
    const FnWs w = fn_ws(n);
    const char* ws = (const char*)workspace;
    hipLaunchKernelGGL(fn_conv1_kernel, dim3((n + 7) / 8), dim3(256), 0, (hipStream_t)stream, feat,
                       reinterpret_cast<const int*>(ws + w.off_perm), reinterpret_cast<const int*>(ws + w.off_nbr), status + 1, W, scale,
                       shift, out);
    UMEREG_CHECK_LAUNCH("fn_conv1_kernel");
    return UMEREG_OK;
}
