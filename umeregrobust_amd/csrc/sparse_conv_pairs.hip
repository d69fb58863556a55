// sparse_conv_pairs.hip -- the pair-compacted engine of the 27-offset sparse convolutions (include/umereg_sparse_conv_pairs.h;
// opt-in, conv_mode="pairs"): for every offset k the matrix unit is fed only the rows of a tile that have a neighbour at k.
//
// fn_conv_kernel (featnet.hip, the "union" engine) walks every offset that SOME row of its tile uses and issues MFMAs for ALL rows
// of the tile; a row without that neighbour stages zeros.  A row has 2-10 neighbours and a tile's union covers nearly all 27
// offsets, so about a fifth of the issued work is useful.  Here a workgroup of 256 threads owns kCpTM = 128 output
// rows x TN output channels (conv_pairs_plan.h) and
//   1. builds once, from the masks, for every offset k the list of its rows that are active at k, ascending (ballot + prefix per
//      wave, no atomics): the row's place in the tile and the neighbour's global row, so the table itself never sits in LDS;
//   2. keeps the tile's accumulators in LDS as f32 [TM][TN], zero at the start;
//   3. walks the offsets with a non-empty list, k ascending, and per offset the 32-channel slices ascending.  The work items of an
//      offset are (block of 32 list slots, 32-column strip), spread over the four waves.  A wave loads the C operand of its item
//      from the accumulator rows its slots name at the first slice, runs the slices' MFMAs on the staged A (the gathered rows of
//      the list's slots: only pairs that exist are loaded) and B (the weight slice), and writes D back after the last slice.
//      Slots past the list's end carry C = 0 and whatever the A tile held; their D rows are discarded (an MFMA's output rows do
//      not depend on each other).  The global loads of step s + 1 are in flight during the MFMAs of step s, as in the union engine;
//   4. applies the union engine's epilogue to every row of the tile: fmaf(acc, scale, shift), residual, ReLU, f16 range flag.
// The rows of the items of one offset are disjoint, and offsets are separated by the barriers the staging needs, so every output
// element is one ordered chain: the union engine's -- same instructions, same slices, offsets ascending, channels ascending --
// minus the links that add 0 * w.  A row with an empty mask keeps acc = 0 and gets its epilogue.  Deterministic, no atomics on
// data, nothing in the workspace.
//
// Two kernel texts, f32 and f16, for the reason featnet.hip's pair has two; the list building, the epilogue and the
// host dispatch are shared.  1x1 layers, conv1 and `final` stay on featnet.hip's kernels in both modes.
#include "conv_pairs_plan.h"
#include "sparse.h"
#include "umereg_featnet_f16.h"

namespace umereg {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
constexpr int kKC = 32;                 // input channels per staged slice
constexpr int kKP = kKC + 8;            // f16 per padded LDS row (featnet.hip)
constexpr float kF16Max = 65504.f;

// per offset k: the tile's active rows, ascending -- slot s of offset k is tile row row[k][s], whose neighbour is input row nbr[k][s]
template <int TM>
struct CpLists {
    int nbr[kFnVol][TM];
    unsigned char row[kFnVol][TM];
    int cnt[kFnVol];
};

// wave w builds the lists of offsets w, w + 4, ...: 64 rows per ballot, a row's slot is the number of active rows before it
template <int TM>
__device__ __forceinline__ void cp_build_lists(CpLists<TM>& L, const ConvArgs& a, int m0, int n_rows, int lane, int wave)
{
    constexpr int CH = TM / 64;
    unsigned int mk[CH];
#pragma unroll
    for (int c = 0; c < CH; ++c) mk[c] = m0 + c * 64 + lane < n_rows ? a.mask[m0 + c * 64 + lane] : 0u;
    for (int k = wave; k < kFnVol; k += 4) {
        int base = 0;
#pragma unroll
        for (int c = 0; c < CH; ++c) {
            const int r = c * 64 + lane;
            const int j = (mk[c] >> k) & 1u ? a.nbr[(size_t)(m0 + r) * kFnVol + k] : -1;
            const unsigned long long on = __ballot(j >= 0);
            if (j >= 0) {
                const int s = base + __popcll(on & ((1ull << lane) - 1ull));
                L.nbr[k][s] = j;
                L.row[k][s] = (unsigned char)r;
            }
            base += __popcll(on);
        }
        if (lane == 0) L.cnt[k] = base;
    }
}

// the union engine's epilogue over the whole tile: thread t owns column t % TN of rows t / TN, t / TN + 256 / TN, ...
template <int TM, int TN, bool F16>
__device__ __forceinline__ void cp_epilogue(const float (&Acc)[TM][TN], const ConvArgs& a, int32_t* range, int m0, int n0, int n_rows, int tid)
{
    const int c = tid % TN, col = n0 + c;
    const float sc = a.scale[col], sh = a.shift[col];
    bool out_of_range = false;
    for (int lr = tid / TN; lr < TM; lr += 256 / TN) {
        const int row = m0 + lr;
        if (row >= n_rows) break;
        float v = fmaf(Acc[lr][c], sc, sh);
        if (a.res) v += a.res[(size_t)row * a.ld_res + col];
        if (F16) out_of_range |= v != v;              // (a NaN, which the ReLU would hide, comes from infinities met on the way)
        if (a.relu) v = fmaxf(v, 0.f);
        if (F16) out_of_range |= fabsf(v) > kF16Max;
        a.out[(size_t)row * a.ld_out + col] = v;
    }
    if (F16 && range && out_of_range) atomicOr(range, UMEREG_FN_ERR_F16_RANGE);
}

template <int TM, int TN>
__global__ __launch_bounds__(kCpThreads) void cp_conv_kernel(ConvArgs a)
{
    constexpr int NS = TN / 32;                 // 32-column strips
    constexpr int NI = (TM / 32) * NS / 4;      // work items per wave and offset, at most
    constexpr int TPR = 256 / TM;               // staging threads per slot
    constexpr int AF = kKC / TPR;               // floats each of them stages
    constexpr int BF = kKC * TN / 256;          // weight floats per thread
    constexpr int BTPR = TN / BF;
    static_assert(TM % 64 == 0 && TM <= 256 && (TM & (TM - 1)) == 0 && NI >= 1 && 4 % NS == 0 && AF % 4 == 0 && BF % 4 == 0 && 256 / BTPR == kKC, "tile shape");
    __shared__ float Acc[TM][TN];
    __shared__ float As[TM][kKC + 1];
    __shared__ __attribute__((aligned(16))) float Bs[kKC][TN];
    __shared__ __attribute__((aligned(16))) CpLists<TM> L;

    const int n_rows = *a.n_out;
    const int m0 = blockIdx.x * TM;
    if (m0 >= n_rows) return;
    const int n0 = blockIdx.y * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave % NS, h = lane >> 5, c32 = lane & 31;
    for (int e = tid; e < TM * TN; e += 256) (&Acc[0][0])[e] = 0.f;
    cp_build_lists<TM>(L, a, m0, n_rows, lane, wave);
    __syncthreads();

    // steps: (offset k, channel slice) over the offsets with a non-empty list, k ascending
    const int lr = tid / TPR, seg = tid % TPR;
    const int br = tid / BTPR, bc = (tid % BTPR) * BF;
    const int n_sl = a.cin / kKC;
    unsigned int rem = (unsigned int)__ballot((lane < kFnVol ? L.cnt[lane] : 0) > 0);
    int k = rem ? __builtin_ctz(rem) : 0, sl = 0;
    float4 av[AF / 4], bv[BF / 4];
    auto load = [&](int k_, int sl_) {
        if (lr < L.cnt[k_]) {
            const float4* p = reinterpret_cast<const float4*>(a.in + (size_t)L.nbr[k_][lr] * a.ld_in + sl_ * kKC + seg * AF);
#pragma unroll
            for (int j = 0; j < AF / 4; ++j) av[j] = p[j];
        }
        const float4* q = reinterpret_cast<const float4*>(a.W + ((size_t)k_ * a.cin + sl_ * kKC + br) * a.cout + n0 + bc);
#pragma unroll
        for (int j = 0; j < BF / 4; ++j) bv[j] = q[j];
    };
    f32x16 acc[NI];
    unsigned int rw[NI][4];                     // the tile rows of the item's slots, four per word
#pragma unroll
    for (int j = 0; j < NI; ++j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) rw[j][q] = 0u;
    }
    if (rem) load(k, sl);
    while (rem) {
        const int P = L.cnt[k];
        __syncthreads();                              // the previous step's LDS tiles are consumed
        if (lr < P) {
#pragma unroll
            for (int j = 0; j < AF / 4; ++j) {
                As[lr][seg * AF + 4 * j + 0] = av[j].x;
                As[lr][seg * AF + 4 * j + 1] = av[j].y;
                As[lr][seg * AF + 4 * j + 2] = av[j].z;
                As[lr][seg * AF + 4 * j + 3] = av[j].w;
            }
        }
#pragma unroll
        for (int j = 0; j < BF / 4; ++j) *reinterpret_cast<float4*>(&Bs[br][bc + 4 * j]) = bv[j];
        __syncthreads();
        const int ck = k;
        const bool first = sl == 0, last = sl + 1 == n_sl;
        if (++sl == n_sl) {
            sl = 0;
            rem &= rem - 1u;
            k = rem ? __builtin_ctz(rem) : 0;
        }
        if (rem) load(k, sl);
        const int nb = cp_blocks(P);
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int b = (wave + 4 * j) / NS;        // item (block b, strip wn)
            if (b >= nb) continue;
            // C/D: col = lane & 31, slot = 32 b + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
            if (first) {
#pragma unroll
                for (int q = 0; q < 4; ++q) rw[j][q] = *reinterpret_cast<const unsigned int*>(&L.row[ck][b * 32 + 8 * q + 4 * h]);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int slot = b * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const int row = (rw[j][r >> 2] >> (8 * (r & 3))) & (TM - 1);
                    acc[j][r] = slot < P ? Acc[row][wn * 32 + c32] : 0.f;
                }
            }
            // lane l: A[slot l & 31][k = l >> 5], B[k = l >> 5][col l & 31]
#pragma unroll
            for (int kk = 0; kk < kKC / 2; ++kk) {
                const float x = As[b * 32 + c32][2 * kk + h];
                const float y = Bs[2 * kk + h][wn * 32 + c32];
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x, y, acc[j], 0, 0, 0);
            }
            if (last) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int slot = b * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const int row = (rw[j][r >> 2] >> (8 * (r & 3))) & (TM - 1);
                    if (slot < P) Acc[row][wn * 32 + c32] = acc[j][r];
                }
            }
        }
    }
    __syncthreads();
    cp_epilogue<TM, TN, false>(Acc, a, nullptr, m0, n0, n_rows, tid);
}

// ---- the f16-operand twin: featnet.hip's fn_conv_f16_kernel is to fn_conv_kernel what this is to cp_conv_kernel --------------------
//
// The staged tiles hold f16 (each gathered activation and each weight rounded to nearest even where the tile is staged), the B tile
// transposed and both padded to 80-byte rows (featnet.hip); a 32-channel step is two v_mfma_f32_32x32x16_f16 with f32 accumulation.
template <int TM, int TN>
__global__ __launch_bounds__(kCpThreads) void cp_conv_f16_kernel(ConvArgsF16 args)
{
    constexpr int NS = TN / 32;                 // 32-column strips
    constexpr int NI = (TM / 32) * NS / 4;      // work items per wave and offset, at most
    constexpr int TPR = 256 / TM;               // staging threads per slot
    constexpr int AF = kKC / TPR;               // activations each of them stages
    constexpr int BF = kKC * TN / 256;          // weights per thread: BF consecutive channels of one output column
    static_assert(TM % 64 == 0 && TM <= 256 && (TM & (TM - 1)) == 0 && NI >= 1 && 4 % NS == 0 && AF % 8 == 0 && (BF == 4 || BF == 8) && (256 / TN) * BF == kKC,
                  "tile shape");
    __shared__ float Acc[TM][TN];
    __shared__ __attribute__((aligned(16))) _Float16 As[TM][kKP];
    __shared__ __attribute__((aligned(16))) _Float16 Bt[TN][kKP];   // Bt[col][channel]
    __shared__ __attribute__((aligned(16))) CpLists<TM> L;

    const ConvArgs& a = args.c;
    const int n_rows = *a.n_out;
    const int m0 = blockIdx.x * TM;
    if (m0 >= n_rows) return;
    const int n0 = blockIdx.y * TN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave % NS, h = lane >> 5, c32 = lane & 31;
    for (int e = tid; e < TM * TN; e += 256) (&Acc[0][0])[e] = 0.f;
    cp_build_lists<TM>(L, a, m0, n_rows, lane, wave);
    __syncthreads();

    // steps: (offset k, channel slice) over the offsets with a non-empty list, k ascending; the loads are f32, as stored, and are
    // rounded when they are staged
    const int lr = tid / TPR, seg = tid % TPR;
    const int bcol = tid % TN, bk = (tid / TN) * BF;
    const int n_sl = a.cin / kKC;
    unsigned int rem = (unsigned int)__ballot((lane < kFnVol ? L.cnt[lane] : 0) > 0);
    int k = rem ? __builtin_ctz(rem) : 0, sl = 0;
    float4 av[AF / 4];
    float bv[BF];
    auto load = [&](int k_, int sl_) {
        if (lr < L.cnt[k_]) {
            const float4* p = reinterpret_cast<const float4*>(a.in + (size_t)L.nbr[k_][lr] * a.ld_in + sl_ * kKC + seg * AF);
#pragma unroll
            for (int j = 0; j < AF / 4; ++j) av[j] = p[j];
        }
        const float* q = a.W + ((size_t)k_ * a.cin + sl_ * kKC + bk) * a.cout + n0 + bcol;
#pragma unroll
        for (int j = 0; j < BF; ++j) bv[j] = q[(size_t)j * a.cout];
    };
    f32x16 acc[NI];
    unsigned int rw[NI][4];                     // the tile rows of the item's slots, four per word
#pragma unroll
    for (int j = 0; j < NI; ++j) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
#pragma unroll
        for (int q = 0; q < 4; ++q) rw[j][q] = 0u;
    }
    if (rem) load(k, sl);
    while (rem) {
        const int P = L.cnt[k];
        __syncthreads();                              // the previous step's LDS tiles are consumed
        if (lr < P) {
#pragma unroll
            for (int j = 0; j < AF / 8; ++j) {
                f16x8 v;
                v[0] = (_Float16)av[2 * j].x, v[1] = (_Float16)av[2 * j].y, v[2] = (_Float16)av[2 * j].z, v[3] = (_Float16)av[2 * j].w;
                v[4] = (_Float16)av[2 * j + 1].x, v[5] = (_Float16)av[2 * j + 1].y, v[6] = (_Float16)av[2 * j + 1].z,
                v[7] = (_Float16)av[2 * j + 1].w;
                *reinterpret_cast<f16x8*>(&As[lr][seg * AF + 8 * j]) = v;
            }
        }
#pragma unroll
        for (int j = 0; j < BF; ++j) Bt[bcol][bk + j] = (_Float16)bv[j];
        __syncthreads();
        const int ck = k;
        const bool first = sl == 0, last = sl + 1 == n_sl;
        if (++sl == n_sl) {
            sl = 0;
            rem &= rem - 1u;
            k = rem ? __builtin_ctz(rem) : 0;
        }
        if (rem) load(k, sl);
        const int nb = cp_blocks(P);
#pragma unroll
        for (int j = 0; j < NI; ++j) {
            const int b = (wave + 4 * j) / NS;        // item (block b, strip wn)
            if (b >= nb) continue;
            // C/D: col = lane & 31, slot = 32 b + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
            if (first) {
#pragma unroll
                for (int q = 0; q < 4; ++q) rw[j][q] = *reinterpret_cast<const unsigned int*>(&L.row[ck][b * 32 + 8 * q + 4 * h]);
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int slot = b * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const int row = (rw[j][r >> 2] >> (8 * (r & 3))) & (TM - 1);
                    acc[j][r] = slot < P ? Acc[row][wn * 32 + c32] : 0.f;
                }
            }
            // lane l (r = l & 31, h = l >> 5): A[slot r][8h + i], B[8h + i][col r], i = 0..7
#pragma unroll
            for (int kk = 0; kk < kKC / 16; ++kk) {
                const f16x8 x = *reinterpret_cast<const f16x8*>(&As[b * 32 + c32][16 * kk + 8 * h]);
                const f16x8 y = *reinterpret_cast<const f16x8*>(&Bt[wn * 32 + c32][16 * kk + 8 * h]);
                acc[j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(x, y, acc[j], 0, 0, 0);
            }
            if (last) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int slot = b * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
                    const int row = (rw[j][r >> 2] >> (8 * (r & 3))) & (TM - 1);
                    if (slot < P) Acc[row][wn * 32 + c32] = acc[j][r];
                }
            }
        }
    }
    __syncthreads();
    cp_epilogue<TM, TN, true>(Acc, a, args.range, m0, n0, n_rows, tid);
}

}  // namespace

int fn_launch_conv_pairs(const ConvArgs& a, bool f16, int32_t* range, int rows_bound, hipStream_t st)
{
    const int tn = cp_tile_cols(a.cout);
    const dim3 grid((rows_bound + kCpTM - 1) / kCpTM, a.cout / tn);
    const ConvArgsF16 h{a, range};
    if (f16 && tn == 64) hipLaunchKernelGGL((cp_conv_f16_kernel<kCpTM, 64>), grid, dim3(kCpThreads), 0, st, h);
    else if (f16) hipLaunchKernelGGL((cp_conv_f16_kernel<kCpTM, 32>), grid, dim3(kCpThreads), 0, st, h);
    else if (tn == 64) hipLaunchKernelGGL((cp_conv_kernel<kCpTM, 64>), grid, dim3(kCpThreads), 0, st, a);
    else hipLaunchKernelGGL((cp_conv_kernel<kCpTM, 32>), grid, dim3(kCpThreads), 0, st, a);
    UMEREG_CHECK_LAUNCH(f16 ? "cp_conv_f16_kernel" : "cp_conv_kernel");
    return UMEREG_OK;
}

}  // namespace umereg
