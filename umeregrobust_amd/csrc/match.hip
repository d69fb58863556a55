// match.hip -- a3/a4/a5 as the caller sees them: bases (ortho.hip) + one of the matchers, and the match probabilities.
// Replaces utils.loc_utils.ume_cdist (reference utils/loc_utils.py:8-15), the row arg-min at evaluate.py:224 and the
// softmax weights at evaluate.py:235-236.  Host composition of the public entries of ume_dist.hip (exact scans) and
// match_f16r.hip (filter + refine); the only kernel here is the softmax.
#include "common.h"
#include "grid.h"
#include "match_dev.h"

namespace umereg {

// a5: a = exp((1 - d)/tau); prob = a / sum(a)   (evaluate.py:235-236), one workgroup
__global__ __launch_bounds__(1024) void match_prob_kernel(const float* __restrict__ d, int n, float tau,
                                                          float* __restrict__ prob)
{
    __shared__ float red[16];
    __shared__ float total;
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float a = expf((1.0f - d[i]) / tau);
        prob[i] = a;
        acc += a;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) acc += __shfl_xor(acc, m, kWave);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.f;
        for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
        total = t;
    }
    __syncthreads();
    const float t = total;
    for (int i = threadIdx.x; i < n; i += blockDim.x) prob[i] = prob[i] / t;
}

}  // namespace umereg

using namespace umereg;

UMEREG_API size_t umereg_ume_cdist_workspace_bytes(int B, int n1, int n2)
{
    if (B <= 0 || n1 <= 0 || n2 <= 0) return 0;
    return qa_bytes(n1) + qb_bytes(n2);
}

UMEREG_API size_t umereg_ume_match_workspace_bytes_ex(int B, int n1, int n2, const umereg_match_opts* opts)
{
    if (B <= 0 || n1 <= 0 || n2 <= 0) return 0;
    MatchOpts o;
    if (resolve_opts(opts, o, "ume_match_workspace_bytes_ex")) return 0;
    return qa_bytes(n1) + qb_bytes(n2) + match_scratch_bytes(n1, n2, o) + 8 * (size_t)n1;   // covers the n1 x 8 B keys of the scan variants
}
UMEREG_API size_t umereg_ume_match_workspace_bytes(int B, int n1, int n2) { return umereg_ume_match_workspace_bytes_ex(B, n1, n2, nullptr); }

UMEREG_API size_t umereg_ume_match_q_scratch_bytes_ex(int n1, int n2, const umereg_match_opts* opts)
{
    MatchOpts o;
    if (n1 <= 0 || n2 <= 0 || resolve_opts(opts, o, "ume_match_q_scratch_bytes_ex")) return 0;
    return match_scratch_bytes(n1, n2, o);
}
UMEREG_API size_t umereg_ume_match_q_scratch_bytes(int n1, int n2) { return umereg_ume_match_q_scratch_bytes_ex(n1, n2, nullptr); }

// (the reset touches the first 4 n1 bytes only -- the per-row limits lead the scratch whatever the options)
UMEREG_API int umereg_ume_match_reset_f16(void* scratch, size_t scratch_bytes, int n1, int n2, void* stream)
{
    UMEREG_REQUIRE(n1 > 0 && n2 > 0, "ume_match_reset_f16: n1, n2 must be positive (got %d, %d)", n1, n2);
    if (int rc = check_device()) return rc;
    if (!scratch || scratch_bytes < (size_t)n1 * sizeof(unsigned int) || ((uintptr_t)scratch & 15)) {
        set_error("ume_match_reset_f16: scratch too small or misaligned (%zu < %zu)", scratch_bytes, (size_t)n1 * sizeof(unsigned int));
        return UMEREG_EWORKSPACE;
    }
#if defined(UMEREG_COARSE_KEEP_LIMITS) && UMEREG_COARSE_KEEP_LIMITS
    // timing experiment (tools/exp_coarse_skip.py on a replayed pair): the coarse pass starts from the limits the previous pass over
    // the SAME pair left behind -- what any publishing schedule can at best approach.  Wrong for any other use.
    return UMEREG_OK;
#endif
    // the per-row limits start at 0; everything else in the scratch is written before it is read
    return launch_zero(scratch, (size_t)n1 * sizeof(unsigned int), 1, 0, (hipStream_t)stream);
}

// order1 / order2: the slot order the bases were written in (MatchScratch, match_dev.h); the coarse pass works on slots and needs none
static int match_q_f16r(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2, int64_t* match_idx, float* match_dist,
                        void* scratch, size_t scratch_bytes, const umereg_match_opts* opts, const int* order1, const int* order2,
                        void* stream)
{
    UMEREG_REQUIRE(match_idx, "ume_match_q_f16r: null match_idx");
    if (int rc = umereg_ume_match_reset_f16(scratch, scratch_bytes, n1, n2, stream)) return rc;
    if (int rc = umereg_ume_match_coarse_f16_ex(Q1_rows_h, Q2_cols_h, n1, n2, scratch, scratch_bytes, opts, stream)) return rc;
    return match_refine_f16(Q1_rows_h, Q2_cols_h, n1, n2, scratch, scratch_bytes, match_idx, match_dist, opts, order1, order2, stream);
}
UMEREG_API int umereg_ume_match_q_f16r_ex(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2,
                                          int64_t* match_idx, float* match_dist, void* scratch, size_t scratch_bytes,
                                          const umereg_match_opts* opts, void* stream)
{
    return match_q_f16r(Q1_rows_h, Q2_cols_h, n1, n2, match_idx, match_dist, scratch, scratch_bytes, opts, nullptr, nullptr, stream);
}
UMEREG_API int umereg_ume_match_q_f16r(const void* Q1_rows_h, const void* Q2_cols_h, int n1, int n2,
                                       int64_t* match_idx, float* match_dist, void* scratch, size_t scratch_bytes,
                                       void* stream)
{
    return umereg_ume_match_q_f16r_ex(Q1_rows_h, Q2_cols_h, n1, n2, match_idx, match_dist, scratch, scratch_bytes, nullptr, stream);
}

static int dist_common(const float* ume1, const float* ume2, int B, int n1, int n2, float* D,
                       int64_t* match_idx, float* match_dist, void* workspace, size_t workspace_bytes,
                       size_t need, void* stream, const char* who, bool f16x2 = false, bool refine = false,
                       const umereg_match_opts* opts = nullptr, const int* order1 = nullptr, const int* order2 = nullptr)
{
    MatchOpts mo;
    if (int rc = resolve_opts(opts, mo, who)) return rc;
    UMEREG_REQUIRE(ume1 && ume2, "%s: null UME pointer", who);
    UMEREG_REQUIRE(B > 0 && n1 > 0 && n2 > 0, "%s: B, n1, n2 must be positive (got %d, %d, %d)", who, B, n1, n2);
    UMEREG_REQUIRE((!order1 && !order2) || (order1 && order2 && refine && B == 1), "%s: a slot order needs both sets, f16r and B = 1", who);
    UMEREG_REQUIRE(((uintptr_t)ume1 & 15) == 0 && ((uintptr_t)ume2 & 15) == 0, "%s: UME pointers must be 16-byte aligned", who);
    if (int rc = check_device()) return rc;
    UMEREG_REQUIRE_WORKSPACE(who, workspace, workspace_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    float* QA = (float*)workspace;
    float* QB = (float*)((char*)workspace + qa_bytes(n1));
    void* keys = (char*)workspace + qa_bytes(n1) + qb_bytes(n2);
    for (int b = 0; b < B; ++b) {
        if (int rc = launch_orthobasis_pair(ume1 + (size_t)b * n1 * 128, n1, f16x2 ? UMEREG_QLAYOUT_ROWS_F16X2 : UMEREG_QLAYOUT_ROWS, QA,
                                            ume2 + (size_t)b * n2 * 128, n2, f16x2 ? UMEREG_QLAYOUT_COLS_F16X2 : UMEREG_QLAYOUT_COLS, QB,
                                            st, order1, order2)) return rc;
        float* Db = D ? D + (size_t)b * n1 * n2 : nullptr;
        int64_t* mi = match_idx ? match_idx + (size_t)b * n1 : nullptr;
        float* md = match_dist ? match_dist + (size_t)b * n1 : nullptr;
        const int rc = refine  ? match_q_f16r(QA, QB, n1, n2, mi, md, keys, match_scratch_bytes(n1, n2, mo), opts, order1, order2, stream)
                       : f16x2 ? umereg_ume_dist_q_f16x2(QA, QB, n1, n2, Db, mi, md, match_idx ? keys : nullptr, stream)
                               : umereg_ume_dist_q_f32(QA, QB, n1, n2, Db, mi, md, match_idx ? keys : nullptr, stream);
        if (rc) return rc;
    }
    return UMEREG_OK;
}

UMEREG_API int umereg_ume_cdist_f32(const float* ume1, const float* ume2, int B, int n1, int n2, float* D,
                                    void* workspace, size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(D, "ume_cdist: null output");
    return dist_common(ume1, ume2, B, n1, n2, D, nullptr, nullptr, workspace, workspace_bytes,
                       umereg_ume_cdist_workspace_bytes(B, n1, n2), stream, "ume_cdist");
}

UMEREG_API int umereg_ume_match_f32(const float* ume1, const float* ume2, int B, int n1, int n2,
                                    int64_t* match_idx, float* match_dist, void* workspace,
                                    size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(match_idx, "ume_match: null match_idx");
    return dist_common(ume1, ume2, B, n1, n2, nullptr, match_idx, match_dist, workspace, workspace_bytes,
                       umereg_ume_match_workspace_bytes(B, n1, n2), stream, "ume_match");
}

UMEREG_API int umereg_match_prob_f32(const float* ume_d, int n, float tau, float* prob, void* stream)
{
    UMEREG_REQUIRE(ume_d && prob, "match_prob: null pointer");
    UMEREG_REQUIRE(n > 0 && tau > 0.f, "match_prob: n and tau must be positive");
    if (int rc = check_device()) return rc;
    hipLaunchKernelGGL(match_prob_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, ume_d, n, tau, prob);
    UMEREG_CHECK_LAUNCH("match_prob_kernel");
    return UMEREG_OK;
}

UMEREG_API int umereg_ume_match_f16x2(const float* ume1, const float* ume2, int B, int n1, int n2,
                                      int64_t* match_idx, float* match_dist, void* workspace,
                                      size_t workspace_bytes, void* stream)
{
    UMEREG_REQUIRE(match_idx, "ume_match_f16x2: null match_idx");
    return dist_common(ume1, ume2, B, n1, n2, nullptr, match_idx, match_dist, workspace, workspace_bytes,
                       umereg_ume_match_workspace_bytes(B, n1, n2), stream, "ume_match_f16x2", true);
}

UMEREG_API int umereg_ume_match_f16r_ex(const float* ume1, const float* ume2, int B, int n1, int n2,
                                        int64_t* match_idx, float* match_dist, void* workspace,
                                        size_t workspace_bytes, const umereg_match_opts* opts, void* stream)
{
    UMEREG_REQUIRE(match_idx, "ume_match_f16r: null match_idx");
    MatchOpts mo;
    if (int rc = resolve_opts(opts, mo, "ume_match_f16r")) return rc;
    return dist_common(ume1, ume2, B, n1, n2, nullptr, match_idx, match_dist, workspace, workspace_bytes,
                       umereg_ume_match_workspace_bytes_ex(B, n1, n2, opts), stream, "ume_match_f16r", true, true, opts);
}
int umereg::match_f16r_ordered(const float* ume1, const float* ume2, int n1, int n2, const int* order1, const int* order2,
                               int64_t* match_idx, float* match_dist, void* workspace, size_t workspace_bytes,
                               const umereg_match_opts* opts, void* stream)
{
    UMEREG_REQUIRE(match_idx, "ume_match_f16r: null match_idx");
    return dist_common(ume1, ume2, 1, n1, n2, nullptr, match_idx, match_dist, workspace, workspace_bytes,
                       umereg_ume_match_workspace_bytes_ex(1, n1, n2, opts), stream, "ume_match_f16r", true, true, opts, order1, order2);
}
UMEREG_API int umereg_ume_match_f16r(const float* ume1, const float* ume2, int B, int n1, int n2,
                                     int64_t* match_idx, float* match_dist, void* workspace,
                                     size_t workspace_bytes, void* stream)
{
    return umereg_ume_match_f16r_ex(ume1, ume2, B, n1, n2, match_idx, match_dist, workspace, workspace_bytes, nullptr, stream);
}
