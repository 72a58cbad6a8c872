// sklearn.preprocessing.StandardScaler on a feature matrix given as up to four COLUMN BLOCKS ("parts": mmvae_standardize_fit,
// mmvae_standardize_apply, include/mmvae_hip.h): the [original | imputed] matrix of the clustering tables is standardised while it is
// assembled and never exists unstandardised.  Both kernels are streaming: one read for the moments, one read and one fp32 write for z.
//
// Thread map: a lane owns ONE column for the whole launch, so a wave reads 64 consecutive elements of a row (256 bytes of fp32) and
// nothing is demanded of a part's alignment, leading dimension or of where a part starts in z (1354 = 782 + 572 columns, bf16 parts
// at odd columns).  What keeps the memory system busy is rows, not vector width: four independent loads per lane are issued before
// the first is used.
//   fit:   workgroup = 64 columns x 4 waves; blockIdx.y = row split; wave w of split s takes the rows r0 + w, r0 + w + 4, ... of the
//          split in ascending order.  a = (double)x - (double)x[0][j] (the column's FIRST ROW is the shift, the same in every split);
//          S0 += a, S1 += a a, all float64.  The four waves meet in LDS and are added in wave order, the split's pair goes to `work`,
//          and a second small launch adds the splits in ascending order: no atomics, every slot of `work` that is read was written
//          by this call.
//   apply: workgroup = 256 columns; mean_j and scale_j sit in the lane's registers; blockIdx.y walks blocks of 16 rows.
#include "common.h"

namespace mm {

constexpr int STD_CT = 64;            // fit: columns per workgroup, one per lane
constexpr int STD_WAVES = 4;          // fit: waves per workgroup = the row interleave inside a split
constexpr int STD_MAX_SPLITS = 64;
constexpr int STD_TARGET_WG = 2048;   // fit: workgroups asked for (8 per CU, 32 waves)
constexpr int STD_AT = 256;           // apply: columns per workgroup
constexpr int STD_AR = 16;            // apply: rows per workgroup step

struct StdPartK { const char* x; long stride; long col0; long cols; int esize; int one_row; };   // stride in BYTES, 0 for a one-row part
struct StdCols { StdPartK part[MMVAE_STD_MAX_PARTS]; int n_parts; long F; };

struct StdColumn { const char* p; long stride; bool is_bf16; bool one_row; };

// column j of the matrix lies in exactly one part
__device__ __forceinline__ StdColumn std_locate(const StdCols& c, long j) {
    StdColumn o{c.part[0].x, c.part[0].stride, c.part[0].esize == 2, c.part[0].one_row != 0};
    long local = j;
#pragma unroll
    for (int i = 1; i < MMVAE_STD_MAX_PARTS; ++i)
        if (i < c.n_parts && j >= c.part[i].col0) {
            o.p = c.part[i].x; o.stride = c.part[i].stride; o.is_bf16 = c.part[i].esize == 2; o.one_row = c.part[i].one_row != 0;
            local = j - c.part[i].col0;
        }
    o.p += local * (o.is_bf16 ? 2 : 4);
    return o;
}

__device__ __forceinline__ double std_load(const StdColumn& c, long row) {
    const char* q = c.p + row * c.stride;
    return c.is_bf16 ? (double)(float)*(const bf16*)q : (double)*(const float*)q;
}

struct StdFitP { StdCols c; int rows; int rps; double* part; };      // part [splits][2][F]

__global__ __launch_bounds__(STD_CT * STD_WAVES) void std_fit_kernel(StdFitP a) {
    __shared__ double sm[2][STD_WAVES][STD_CT];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, s = blockIdx.y;
    const long j = (long)blockIdx.x * STD_CT + lane;
    const bool live = j < a.c.F;
    double s0 = 0.0, s1 = 0.0;
    if (live) {
        const StdColumn col = std_locate(a.c, j);
        if (!col.one_row) {                                            // a one-row part: every deviation is exactly 0
            const double c = std_load(col, 0);
            const long r0 = (long)s * a.rps, r1 = r0 + a.rps < a.rows ? r0 + a.rps : (long)a.rows;
            long r = r0 + wave;
            for (; r + 3 * STD_WAVES < r1; r += 4 * STD_WAVES) {
                const double x0 = std_load(col, r), x1 = std_load(col, r + STD_WAVES), x2 = std_load(col, r + 2 * STD_WAVES),
                             x3 = std_load(col, r + 3 * STD_WAVES);
                const double a0 = x0 - c, a1 = x1 - c, a2 = x2 - c, a3 = x3 - c;
                s0 += a0; s1 += a0 * a0;
                s0 += a1; s1 += a1 * a1;
                s0 += a2; s1 += a2 * a2;
                s0 += a3; s1 += a3 * a3;
            }
            for (; r < r1; r += STD_WAVES) { const double d = std_load(col, r) - c; s0 += d; s1 += d * d; }
        }
    }
    sm[0][wave][lane] = s0; sm[1][wave][lane] = s1;
    __syncthreads();
    if (wave == 0 && live) {
        double t0 = sm[0][0][lane], t1 = sm[1][0][lane];
#pragma unroll
        for (int w = 1; w < STD_WAVES; ++w) { t0 += sm[0][w][lane]; t1 += sm[1][w][lane]; }
        a.part[((long)s * 2 + 0) * a.c.F + j] = t0;
        a.part[((long)s * 2 + 1) * a.c.F + j] = t1;
    }
}

struct StdFinP { StdCols c; int rows; int splits; const double* part; double* mean; double* var; double* scale; };

__global__ __launch_bounds__(256) void std_finalize_kernel(StdFinP a) {
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= a.c.F) return;
    const StdColumn col = std_locate(a.c, j);
    double S0 = 0.0, S1 = 0.0;
    for (int s = 0; s < a.splits; ++s) { S0 += a.part[((long)s * 2 + 0) * a.c.F + j]; S1 += a.part[((long)s * 2 + 1) * a.c.F + j]; }
    const double n = (double)a.rows, c = std_load(col, 0);
    const double d = S0 / n, mean = c + d;
    double var = S1 / n - d * d;
    if (!(var > 0.0)) var = 0.0;                                       // a population variance is not negative
    // sklearn's _is_constant_feature: the variance is zero up to the rounding of the mean
    const double eps = 2.220446049250313e-16;
    const double t = n * mean * eps, bound = n * eps * var + t * t;
    a.mean[j] = mean; a.var[j] = var; a.scale[j] = var <= bound ? 1.0 : sqrt(var);
}

struct StdApplyP { StdCols c; int rows; const double* mean; const double* scale; float* z; long ldz; };

__global__ __launch_bounds__(STD_AT) void std_apply_kernel(StdApplyP a) {
#pragma clang fp contract(off)
    const long j = (long)blockIdx.x * STD_AT + threadIdx.x;
    if (j >= a.c.F) return;
    const StdColumn col = std_locate(a.c, j);
    const double m = a.mean[j], sc = a.scale[j];
    float* zc = a.z + j;
    const long nrb = ((long)a.rows + STD_AR - 1) / STD_AR;
    for (long rb = blockIdx.y; rb < nrb; rb += gridDim.y) {
        const long r0 = rb * STD_AR, r1 = r0 + STD_AR < a.rows ? r0 + STD_AR : (long)a.rows;
        long r = r0;
        for (; r + 3 < r1; r += 4) {
            const double x0 = std_load(col, r), x1 = std_load(col, r + 1), x2 = std_load(col, r + 2), x3 = std_load(col, r + 3);
            zc[r * a.ldz] = (float)((x0 - m) / sc);
            zc[(r + 1) * a.ldz] = (float)((x1 - m) / sc);
            zc[(r + 2) * a.ldz] = (float)((x2 - m) / sc);
            zc[(r + 3) * a.ldz] = (float)((x3 - m) / sc);
        }
        for (; r < r1; ++r) zc[r * a.ldz] = (float)((std_load(col, r) - m) / sc);
    }
}

// the parts of a call, checked; *any_matrix: at least one part is a (rows, cols) matrix
static int std_cols(const mmvae_std_part* part, int n_parts, StdCols& c, bool& any_matrix) {
    if (n_parts < 1 || n_parts > MMVAE_STD_MAX_PARTS) return MMVAE_ERR_ARG;
    c = StdCols{};
    c.n_parts = n_parts;
    any_matrix = false;
    long F = 0;
    for (int i = 0; i < n_parts; ++i) {
        const mmvae_std_part& p = part[i];
        if (p.dtype != MMVAE_F32 && p.dtype != MMVAE_BF16) return MMVAE_ERR_DTYPE;
        const int es = p.dtype == MMVAE_BF16 ? 2 : 4;
        if (!p.x || ((uintptr_t)p.x % es) || p.cols < 1) return MMVAE_ERR_ARG;
        if (!p.one_row && p.ld < p.cols) return MMVAE_ERR_ARG;
        any_matrix |= !p.one_row;
        c.part[i] = StdPartK{(const char*)p.x, p.one_row ? 0L : (long)p.ld * es, F, (long)p.cols, es, p.one_row ? 1 : 0};
        F += p.cols;
    }
    c.F = F;
    return MMVAE_OK;
}

static int std_plan(int rows, long F, int splits, int& used, int& rps) {
    if (rows < 1 || F < 1 || splits < 0 || splits > STD_MAX_SPLITS) return MMVAE_ERR_ARG;
    const long ctiles = (F + STD_CT - 1) / STD_CT;
    long want = splits;
    if (want == 0) {
        want = STD_TARGET_WG / ctiles;
        if (want > rows / 32) want = rows / 32;
        if (want < 1) want = 1;
    }
    if (want > STD_MAX_SPLITS) want = STD_MAX_SPLITS;
    if (want > rows) want = rows;
    rps = (int)(((long)rows + want - 1) / want);
    used = (int)(((long)rows + rps - 1) / rps);
    return MMVAE_OK;
}

}  // namespace mm

extern "C" int mmvae_standardize_fit_splits(int32_t rows, int64_t F, int32_t splits, int32_t* splits_used) {
    int used, rps;
    if (!splits_used) return MMVAE_ERR_ARG;
    { const int rc = mm::std_plan(rows, F, splits, used, rps); if (rc) return rc; }
    *splits_used = used;
    return MMVAE_OK;
}

extern "C" int mmvae_standardize_fit_work_bytes(int32_t rows, int64_t F, int32_t splits, int64_t* bytes) {
    int used, rps;
    if (!bytes) return MMVAE_ERR_ARG;
    { const int rc = mm::std_plan(rows, F, splits, used, rps); if (rc) return rc; }
    *bytes = 16 * (int64_t)F * used;
    return MMVAE_OK;
}

extern "C" int mmvae_standardize_fit(const mmvae_standardize_fit_args* a, void* stream) {
    using namespace mm;
    if (!a) return MMVAE_ERR_ARG;
    StdCols c; bool any_matrix; int used, rps;
    { const int rc = std_cols(a->part, a->n_parts, c, any_matrix); if (rc) return rc; }
    if (!any_matrix) return MMVAE_ERR_ARG;
    { const int rc = std_plan(a->rows, c.F, a->splits, used, rps); if (rc) return rc; }
    if (!a->mean || !a->var || !a->scale || !a->work) return MMVAE_ERR_ARG;
    if (((uintptr_t)a->mean | (uintptr_t)a->var | (uintptr_t)a->scale | (uintptr_t)a->work) & 7) return MMVAE_ERR_ARG;
    if (a->work_bytes < 16 * (int64_t)c.F * used) return MMVAE_ERR_ARG;
    const long ctiles = (c.F + STD_CT - 1) / STD_CT;
    hipStream_t st = (hipStream_t)stream;
    StdFitP f{c, a->rows, rps, (double*)a->work};
    hipLaunchKernelGGL(std_fit_kernel, dim3((unsigned)ctiles, (unsigned)used), dim3(STD_CT * STD_WAVES), 0, st, f);
    MM_CHECK_LAUNCH();
    StdFinP g{c, a->rows, used, (const double*)a->work, a->mean, a->var, a->scale};
    hipLaunchKernelGGL(std_finalize_kernel, dim3((unsigned)((c.F + 255) / 256)), dim3(256), 0, st, g);
    MM_CHECK_LAUNCH();
    return MMVAE_OK;
}

extern "C" int mmvae_standardize_apply(const mmvae_standardize_apply_args* a, void* stream) {
    using namespace mm;
    if (!a) return MMVAE_ERR_ARG;
    StdCols c; bool any_matrix;
    { const int rc = std_cols(a->part, a->n_parts, c, any_matrix); if (rc) return rc; }
    if (a->rows < 1 || !a->mean || !a->scale || !a->z || a->ldz < c.F) return MMVAE_ERR_ARG;
    if ((((uintptr_t)a->mean | (uintptr_t)a->scale) & 7) || ((uintptr_t)a->z & 3)) return MMVAE_ERR_ARG;
    const long ctiles = (c.F + STD_AT - 1) / STD_AT, nrb = ((long)a->rows + STD_AR - 1) / STD_AR;
    StdApplyP p{c, a->rows, a->mean, a->scale, a->z, (long)a->ldz};
    hipLaunchKernelGGL(std_apply_kernel, dim3((unsigned)ctiles, (unsigned)(nrb < 65535 ? nrb : 65535)), dim3(STD_AT), 0, (hipStream_t)stream, p);
    MM_CHECK_LAUNCH();
    return MMVAE_OK;
}
