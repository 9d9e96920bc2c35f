// Batched sparse solvers (gko::batch): many small systems that share ONE sparsity pattern, every item with its
// own values, right-hand side and solution.
//   batch_plan                         host only: width, LDS residency and workspace of a solve
//   solve_kernel                       batch::solver::Cg / Bicgstab on batch::matrix::Csr / Ell, M = I or scalar Jacobi
//   apply / advanced_apply             x = A b, x = alpha A b + beta x on items x rows x cols multi-vectors
//   scale / add_scaled / dot / norm2   batch::MultiVector
//   csr_to_ell_values / ell_to_csr_values, csr_check / ell_check
//
// Contract: include/gko_cdna4.h, "Batched solvers" (tests/batch_refs.py restates it in numpy).  Every multiply,
// add, subtract, divide and sqrt is a separate operation in T (-ffp-contract=off), a row of a product is the
// sequential sum from +0 over its stored entries, and every dot / norm is the reduction R_W below, so a solve is
// bit-identical to the numpy restatement: x, iteration count, residual norm and converged flag.
//
// The solve is ONE launch, one workgroup of W threads per item; thread l owns the rows l, l + W, ...  Every
// element-wise step touches own rows only; a product gathers its input from all rows, so a barrier stands
// before every product, and the barrier inside the reduction that follows a product keeps its input from being
// overwritten early.  Vectors are addressed through flat pointers: the first `resident` of the solver's fixed
// order live in LDS, the others in the caller's workspace (x: in the caller's x itself), the code is the same.
//
// Invariants:
//   1. no atomics, no waiting between workgroups: an item's workgroup reads the shared pattern and its own
//      slices of values, b, x and the workspace, and writes its own slices of x, the workspace and the outputs;
//   2. every loop that contains a barrier has a trip count that is uniform across the workgroup: all threads
//      hold the same bits of every reduction (every wave reduces the same W partials in the same order);
//   3. the hot entries check host arguments only and never synchronise; the pattern is checked once, by
//      gkoc_batch_csr_check_i32 / gkoc_batch_ell_check_i32, when a batch matrix is made;
//   4. every index pointer is const: no entry writes an index array, none belongs to the column-offset plan.
#include <hip/hip_runtime.h>

#include "common.hpp"

namespace gkoc {
namespace {

constexpr int batch_block = 256;           // the element-wise kernels
// half of a CU's LDS, so that two workgroups share a CU: measured against all of it (one workgroup per CU),
// a third and a quarter
constexpr int64_t batch_lds_budget = 81920;

// measured: 512 threads lose up to 768 rows and win beyond 1024
inline int batch_width(int64_t n) { return n <= 64 ? 64 : n <= 128 ? 128 : n <= 768 ? 256 : 512; }

inline int64_t round16(int64_t bytes) { return (bytes + 15) / 16 * 16; }

// the vectors of a solver in residency order (the header states it); x is always the last one
//   Cg:        p r t [z dinv] x            Bicgstab: [p_hat s_hat] p s r r_hat v t [dinv] x
inline int batch_vector_count(int solver, int precond)
{
    return solver == GKOC_BATCH_CG ? (precond == GKOC_BATCH_JACOBI ? 6 : 4) : (precond == GKOC_BATCH_JACOBI ? 10 : 7);
}

int make_plan(int solver, int format, int precond, int value_bytes, int64_t n, int64_t stored,
              gkoc_batch_plan_info* plan)
{
    GKOC_REQUIRE(plan, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(solver == GKOC_BATCH_CG || solver == GKOC_BATCH_BICGSTAB, GKOC_E_INVALID, "unknown solver");
    GKOC_REQUIRE(format == GKOC_BATCH_CSR || format == GKOC_BATCH_ELL, GKOC_E_INVALID, "unknown format");
    GKOC_REQUIRE(precond == GKOC_BATCH_IDENTITY || precond == GKOC_BATCH_JACOBI, GKOC_E_INVALID,
                 "unknown preconditioner");
    GKOC_REQUIRE(value_bytes == 4 || value_bytes == 8, GKOC_E_INVALID, "the value size is 4 or 8 bytes");
    GKOC_REQUIRE(n >= 0 && stored >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(n <= INT32_MAX, GKOC_E_INVALID, "more rows than a 32-bit index holds");
    const int w = batch_width(n);
    const int total = batch_vector_count(solver, precond);
    const int64_t red = 2 * int64_t(w) * value_bytes;
    const int64_t vec = round16(n * value_bytes);
    const int64_t room = batch_lds_budget - red;
    const int64_t fit = vec == 0 ? total : room / vec;
    const int resident = int(fit < total ? fit : total);
    plan->w = w;
    plan->resident_vectors = resident;
    plan->total_vectors = total;
    plan->values_cached = 0;    // measured and rejected: the copy costs workgroups per CU
    plan->lds_bytes = red + resident * vec;
    // x is the last vector of the order and is updated in the caller's array when it is not resident
    plan->workspace_bytes = resident < total ? (total - resident - 1) * vec : 0;
    return GKOC_OK;
}

// ------------------------------------------------------------------ R_W
// R_W of one partial per thread, the same bits in every thread.  red: 2 * W values; `half` alternates so that
// one barrier per reduction is enough (a thread is never two reductions ahead of another).
template <typename T>
__device__ __forceinline__ T reduce_w(T part, T* red, int& half, int w)
{
    T* buf = red + half * w;
    half ^= 1;
    buf[threadIdx.x] = part;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    T v;
    if (w == 512) {    // d = 256, then d = 128, then d = 64
        v = ((buf[lane] + buf[lane + 256]) + (buf[lane + 128] + buf[lane + 384])) +
            ((buf[lane + 64] + buf[lane + 320]) + (buf[lane + 192] + buf[lane + 448]));
    } else if (w == 256) {    // d = 128, then d = 64
        v = (buf[lane] + buf[lane + 128]) + (buf[lane + 64] + buf[lane + 192]);
    } else if (w == 128) {
        v = buf[lane] + buf[lane + 64];
    } else {
        v = buf[lane];
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = v + __shfl_down(v, d, 64);
    return __shfl(v, 0, 64);
}

template <typename T>
__device__ __forceinline__ T dot_w(int n, const T* u, const T* v, T* red, int& half, int w)
{
    T acc = T(0);
    for (int i = threadIdx.x; i < n; i += w) acc = acc + u[i] * v[i];
    return reduce_w(acc, red, half, w);
}

template <typename T>
__device__ __forceinline__ T nrm_w(int n, const T* u, T* red, int& half, int w)
{
    return sqrt(dot_w(n, u, u, red, half, w));
}

// ------------------------------------------------------------------ the solve
template <typename T>
struct solve_args {
    int n;
    int64_t stored;          // values per item
    const int32_t* rp;       // Csr
    const int32_t* ci;       // Csr: col_idxs, Ell: the column-major slots
    int ell_k;
    int64_t ell_stride;
    const T* vals;
    const T* b;
    int64_t ldb;
    T* x;
    int64_t ldx;
    double tol;
    int relative;
    int max_it;
    T* work;
    int64_t work_elems;      // per item
    int64_t vec_elems;       // spacing of the vectors in LDS and in the workspace
    int resident;
    int* iters;
    T* res;
    int* conv;
};

// row i of A u; u is read at u[c * us]
template <int FMT, typename T>
__device__ __forceinline__ T row_product(const solve_args<T>& a, const T* vals, int i, const T* u, int64_t us)
{
    T acc = T(0);
    if (FMT == GKOC_BATCH_CSR) {
        const int end = a.rp[i + 1];
        for (int e = a.rp[i]; e < end; ++e) acc = acc + vals[e] * u[a.ci[e] * us];
    } else {
        for (int k = 0; k < a.ell_k; ++k) {
            const int64_t at = i + k * a.ell_stride;
            const int c = a.ci[at];
            if (c >= 0) acc = acc + vals[at] * u[c * us];
        }
    }
    return acc;
}

// 1 / a_ii of the first stored entry (i, i); 1 where none is stored or it is 0
template <int FMT, typename T>
__device__ __forceinline__ T jacobi_entry(const solve_args<T>& a, const T* vals, int i)
{
    T d = T(0);
    if (FMT == GKOC_BATCH_CSR) {
        const int end = a.rp[i + 1];
        for (int e = a.rp[i]; e < end; ++e) {
            if (a.ci[e] == i) {
                d = vals[e];
                break;
            }
        }
    } else {
        for (int k = 0; k < a.ell_k; ++k) {
            const int64_t at = i + k * a.ell_stride;
            if (a.ci[at] == i) {
                d = vals[at];
                break;
            }
        }
    }
    return d == T(0) ? T(1) : T(1) / d;
}

template <typename T>
__device__ __forceinline__ bool stops(T res, T tau, int it, int max_it)
{
    return res <= tau || res != res || it == max_it;
}

template <int SOLVER, int FMT, int PRE, typename T>
__global__ __launch_bounds__(512) void solve_kernel(const solve_args<T> a)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr bool JAC = PRE == GKOC_BATCH_JACOBI;
    constexpr int total = SOLVER == GKOC_BATCH_CG ? (JAC ? 6 : 4) : (JAC ? 10 : 7);
    const int w = blockDim.x, n = a.n, tid = threadIdx.x;
    const int64_t item = blockIdx.x;
    T* red = reinterpret_cast<T*>(smem);
    T* lds_vecs = red + 2 * w;
    int half = 0;

    // the first `resident` vectors of the order in LDS, the others in the workspace; x (the last) in place
    T* vec[total];
#pragma unroll
    for (int k = 0; k < total; ++k) {
        vec[k] = k < a.resident ? lds_vecs + k * a.vec_elems
                                : a.work + item * a.work_elems + (k - a.resident) * a.vec_elems;
    }
    const bool x_resident = a.resident == total;
    T* xg = a.x + item * n * a.ldx;
    T* x = x_resident ? vec[total - 1] : xg;
    const int64_t xs = x_resident ? 1 : a.ldx;
    const T* b = a.b + item * n * a.ldb;
    const T* vals = a.vals + item * a.stored;
    if (x_resident) {
        for (int i = tid; i < n; i += w) x[i] = xg[i * a.ldx];
    }
    __syncthreads();

    T tau = T(a.tol);
    if (a.relative) {
        T acc = T(0);
        for (int i = tid; i < n; i += w) acc = acc + b[i * a.ldb] * b[i * a.ldb];
        tau = tau * sqrt(reduce_w(acc, red, half, w));
    }
    int it = 0;
    T res;

    if (SOLVER == GKOC_BATCH_CG) {
        T* p = vec[0];
        T* r = vec[1];
        T* t = vec[2];
        T* z = JAC ? vec[3] : r;
        T* dinv = JAC ? vec[4] : nullptr;
        for (int i = tid; i < n; i += w) {
            if (JAC) dinv[i] = jacobi_entry<FMT>(a, vals, i);
            r[i] = b[i * a.ldb] - row_product<FMT>(a, vals, i, x, xs);
            if (JAC) z[i] = dinv[i] * r[i];
            p[i] = z[i];
        }
        T rho = dot_w(n, r, z, red, half, w);
        res = nrm_w(n, r, red, half, w);
        while (!stops(res, tau, it, a.max_it)) {
            __syncthreads();
            for (int i = tid; i < n; i += w) t[i] = row_product<FMT>(a, vals, i, p, 1);
            const T alpha = rho / dot_w(n, p, t, red, half, w);
            for (int i = tid; i < n; i += w) {
                x[i * xs] = x[i * xs] + alpha * p[i];
                r[i] = r[i] - alpha * t[i];
            }
            res = nrm_w(n, r, red, half, w);
            ++it;
            if (stops(res, tau, it, a.max_it)) break;
            if (JAC) {
                for (int i = tid; i < n; i += w) z[i] = dinv[i] * r[i];
            }
            const T rho_new = dot_w(n, r, z, red, half, w);
            const T beta = rho_new / rho;
            for (int i = tid; i < n; i += w) p[i] = z[i] + beta * p[i];
            rho = rho_new;
        }
    } else {
        constexpr int o = JAC ? 2 : 0;
        T* p = vec[o];
        T* s = vec[o + 1];
        T* r = vec[o + 2];
        T* r_hat = vec[o + 3];
        T* v = vec[o + 4];
        T* t = vec[o + 5];
        T* p_hat = JAC ? vec[0] : p;
        T* s_hat = JAC ? vec[1] : s;
        T* dinv = JAC ? vec[8] : nullptr;
        for (int i = tid; i < n; i += w) {
            if (JAC) dinv[i] = jacobi_entry<FMT>(a, vals, i);
            const T ri = b[i * a.ldb] - row_product<FMT>(a, vals, i, x, xs);
            r[i] = ri;
            r_hat[i] = ri;
            p[i] = T(0);
            v[i] = T(0);
        }
        T rho_old = T(1), alpha = T(1), omega = T(1);
        res = nrm_w(n, r, red, half, w);
        while (!stops(res, tau, it, a.max_it)) {
            const T rho = dot_w(n, r_hat, r, red, half, w);
            const T beta = (rho / rho_old) * (alpha / omega);
            for (int i = tid; i < n; i += w) {
                p[i] = r[i] + beta * (p[i] - omega * v[i]);
                if (JAC) p_hat[i] = dinv[i] * p[i];
            }
            __syncthreads();
            for (int i = tid; i < n; i += w) v[i] = row_product<FMT>(a, vals, i, p_hat, 1);
            alpha = rho / dot_w(n, r_hat, v, red, half, w);
            for (int i = tid; i < n; i += w) s[i] = r[i] - alpha * v[i];
            res = nrm_w(n, s, red, half, w);
            if (res <= tau || res != res) {
                for (int i = tid; i < n; i += w) x[i * xs] = x[i * xs] + alpha * p_hat[i];
                ++it;
                break;
            }
            if (JAC) {
                for (int i = tid; i < n; i += w) s_hat[i] = dinv[i] * s[i];
            }
            __syncthreads();
            for (int i = tid; i < n; i += w) t[i] = row_product<FMT>(a, vals, i, s_hat, 1);
            const T ts = dot_w(n, t, s, red, half, w);
            omega = ts / dot_w(n, t, t, red, half, w);
            for (int i = tid; i < n; i += w) {
                x[i * xs] = (x[i * xs] + alpha * p_hat[i]) + omega * s_hat[i];
                r[i] = s[i] - omega * t[i];
            }
            res = nrm_w(n, r, red, half, w);
            rho_old = rho;
            ++it;
        }
    }
    if (x_resident) {
        for (int i = tid; i < n; i += w) xg[i * a.ldx] = x[i];
    }
    if (tid == 0) {
        a.iters[item] = it;
        a.res[item] = res;
        a.conv[item] = res <= tau ? 1 : 0;
    }
}

template <int SOLVER, int FMT, int PRE, typename T>
int solve_launch(hipStream_t st, int64_t items, const solve_args<T>& a, const gkoc_batch_plan_info& plan)
{
    auto kernel = solve_kernel<SOLVER, FMT, PRE, T>;
    if (plan.lds_bytes > 65536) {
        // more dynamic LDS than the default limit of a launch: raised once per kernel
        static std::atomic<int> raised{0};
        if (raised.load(std::memory_order_relaxed) == 0) {
            GKOC_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, int(batch_lds_budget)));
            raised.store(1, std::memory_order_relaxed);
        }
    }
    kernel<<<dim3(unsigned(items)), dim3(unsigned(plan.w)), size_t(plan.lds_bytes), st>>>(a);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <int SOLVER, int FMT, typename T>
int solve(gkoc_stream_t s, int64_t items, int64_t n, int64_t stored, const int32_t* rp, const int32_t* ci,
          int64_t ell_k, int64_t ell_stride, const T* vals, int precond, const T* b, int64_t ldb, T* x,
          int64_t ldx, double tol, int tol_type, int64_t max_it, void* work, size_t work_bytes, int* iters, T* res,
          int* conv)
{
    GKOC_REQUIRE(items >= 0 && n >= 0 && stored >= 0 && max_it >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(items <= INT32_MAX && n <= INT32_MAX && max_it <= INT32_MAX && stored <= INT32_MAX, GKOC_E_INVALID,
                 "a size beyond 32 bits");
    GKOC_REQUIRE(precond == GKOC_BATCH_IDENTITY || precond == GKOC_BATCH_JACOBI, GKOC_E_INVALID,
                 "unknown preconditioner");
    GKOC_REQUIRE(tol_type == GKOC_BATCH_ABSOLUTE || tol_type == GKOC_BATCH_RELATIVE, GKOC_E_INVALID,
                 "unknown tolerance type");
    GKOC_REQUIRE(ldb >= 1 && ldx >= 1, GKOC_E_INVALID, "a stride smaller than the number of columns");
    if (FMT == GKOC_BATCH_ELL) {
        GKOC_REQUIRE(ell_k >= 0 && ell_stride >= n && stored == ell_k * ell_stride, GKOC_E_INVALID,
                     "a stride smaller than the number of rows, or stored entries that are not slots x stride");
    }
    if (items == 0) return GKOC_OK;
    GKOC_REQUIRE(iters && res && conv, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(n == 0 || (b && x), GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(FMT == GKOC_BATCH_ELL || rp, GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(stored == 0 || (ci && vals), GKOC_E_INVALID, "null pointer");
    gkoc_batch_plan_info plan;
    GKOC_TRY(make_plan(SOLVER, FMT, precond, int(sizeof(T)), n, stored, &plan));
    GKOC_REQUIRE(plan.workspace_bytes == 0 || work, GKOC_E_INVALID, "null workspace");
    GKOC_REQUIRE(plan.workspace_bytes == 0 || work_bytes / size_t(plan.workspace_bytes) >= size_t(items),
                 GKOC_E_INVALID, "a workspace smaller than the plan's");
    solve_args<T> a;
    a.n = int(n);
    a.stored = stored;
    a.rp = rp;
    a.ci = ci;
    a.ell_k = int(ell_k);
    a.ell_stride = ell_stride;
    a.vals = vals;
    a.b = b;
    a.ldb = ldb;
    a.x = x;
    a.ldx = ldx;
    a.tol = tol;
    a.relative = tol_type == GKOC_BATCH_RELATIVE;
    a.max_it = int(max_it);
    a.work = static_cast<T*>(work);
    a.work_elems = plan.workspace_bytes / int64_t(sizeof(T));
    a.vec_elems = round16(n * int64_t(sizeof(T))) / int64_t(sizeof(T));
    a.resident = plan.resident_vectors;
    a.iters = iters;
    a.res = res;
    a.conv = conv;
    hipStream_t st = as_stream(s);
    if (precond == GKOC_BATCH_JACOBI) return solve_launch<SOLVER, FMT, GKOC_BATCH_JACOBI, T>(st, items, a, plan);
    return solve_launch<SOLVER, FMT, GKOC_BATCH_IDENTITY, T>(st, items, a, plan);
}

// ------------------------------------------------------------------ apply
inline unsigned flat_grid(int64_t total) { return stream_grid(total, batch_block); }

// one thread per (item, row, col): x = A b, or x = alpha[item] * (A b) + beta[item] * x
template <int FMT, bool ADVANCED, typename T>
__global__ __launch_bounds__(batch_block) void apply_kernel(int64_t items, int64_t n_rows, int64_t n_cols,
                                                            int64_t stored, const int32_t* __restrict__ rp,
                                                            const int32_t* __restrict__ ci, int64_t ell_k,
                                                            int64_t ell_stride, const T* __restrict__ vals,
                                                            const T* __restrict__ alpha, const T* __restrict__ b,
                                                            int64_t ldb, const T* __restrict__ beta, T* x,
                                                            int64_t ldx, int64_t cols)
{
    const int64_t total = items * n_rows * cols;
    const int64_t step = int64_t(gridDim.x) * batch_block;
    for (int64_t idx = int64_t(blockIdx.x) * batch_block + threadIdx.x; idx < total; idx += step) {
        const int64_t col = idx % cols;
        const int64_t row = (idx / cols) % n_rows;
        const int64_t item = idx / (cols * n_rows);
        const T* v = vals + item * stored;
        const T* bi = b + item * n_cols * ldb + col;
        T acc = T(0);
        if (FMT == GKOC_BATCH_CSR) {
            const int64_t end = rp[row + 1];
            for (int64_t e = rp[row]; e < end; ++e) acc = acc + v[e] * bi[int64_t(ci[e]) * ldb];
        } else {
            for (int64_t k = 0; k < ell_k; ++k) {
                const int64_t at = row + k * ell_stride;
                const int64_t c = ci[at];
                if (c >= 0) acc = acc + v[at] * bi[c * ldb];
            }
        }
        T* out = x + (item * n_rows + row) * ldx + col;
        if (ADVANCED) {
            *out = alpha[item] * acc + beta[item] * *out;
        } else {
            *out = acc;
        }
    }
}

template <int FMT, bool ADVANCED, typename T>
int apply(gkoc_stream_t s, int64_t items, int64_t n_rows, int64_t n_cols, int64_t stored, const int32_t* rp,
          const int32_t* ci, int64_t ell_k, int64_t ell_stride, const T* vals, const T* alpha, const T* b,
          int64_t ldb, const T* beta, T* x, int64_t ldx, int64_t cols)
{
    GKOC_REQUIRE(items >= 0 && n_rows >= 0 && n_cols >= 0 && stored >= 0 && cols >= 0, GKOC_E_INVALID,
                 "negative size");
    GKOC_REQUIRE(ldb >= cols && ldx >= cols, GKOC_E_INVALID, "a stride smaller than the number of columns");
    if (FMT == GKOC_BATCH_ELL) {
        GKOC_REQUIRE(ell_k >= 0 && ell_stride >= n_rows && stored == ell_k * ell_stride, GKOC_E_INVALID,
                     "a stride smaller than the number of rows, or stored entries that are not slots x stride");
    }
    if (items == 0 || n_rows == 0 || cols == 0) return GKOC_OK;
    GKOC_REQUIRE(x && (FMT == GKOC_BATCH_ELL || rp), GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(stored == 0 || (ci && vals && b), GKOC_E_INVALID, "null pointer");
    GKOC_REQUIRE(!ADVANCED || (alpha && beta), GKOC_E_INVALID, "null pointer");
    apply_kernel<FMT, ADVANCED, T><<<dim3(flat_grid(items * n_rows * cols)), dim3(batch_block), 0, as_stream(s)>>>(
        items, n_rows, n_cols, stored, rp, ci, ell_k, ell_stride, vals, alpha, b, ldb, beta, x, ldx, cols);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

// ------------------------------------------------------------------ multi-vector
// x = alpha x (B == nullptr) or x = x + alpha b; alpha[item, alpha_cols == 1 ? 0 : col]
template <bool ADD, typename T>
__global__ __launch_bounds__(batch_block) void scale_kernel(int64_t items, int64_t rows, int64_t cols,
                                                            const T* __restrict__ alpha, int64_t alpha_cols,
                                                            const T* __restrict__ b, int64_t ldb, T* x, int64_t ldx)
{
    const int64_t total = items * rows * cols;
    const int64_t step = int64_t(gridDim.x) * batch_block;
    for (int64_t idx = int64_t(blockIdx.x) * batch_block + threadIdx.x; idx < total; idx += step) {
        const int64_t col = idx % cols;
        const int64_t row = (idx / cols) % rows;
        const int64_t item = idx / (cols * rows);
        const T al = alpha[item * alpha_cols + (alpha_cols == 1 ? 0 : col)];
        T* out = x + (item * rows + row) * ldx + col;
        if (ADD) {
            *out = *out + al * b[(item * rows + row) * ldb + col];
        } else {
            *out = al * *out;
        }
    }
}

template <bool ADD, typename T>
int scale(gkoc_stream_t s, int64_t items, int64_t rows, int64_t cols, const T* alpha, int64_t alpha_cols, const T* b,
          int64_t ldb, T* x, int64_t ldx)
{
    GKOC_REQUIRE(items >= 0 && rows >= 0 && cols >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(alpha_cols == 1 || alpha_cols == cols, GKOC_E_INVALID, "one scalar per item or one per column");
    GKOC_REQUIRE(ldx >= cols && (!ADD || ldb >= cols), GKOC_E_INVALID, "a stride smaller than the number of columns");
    if (items == 0 || rows == 0 || cols == 0) return GKOC_OK;
    GKOC_REQUIRE(alpha && x && (!ADD || b), GKOC_E_INVALID, "null pointer");
    scale_kernel<ADD, T><<<dim3(flat_grid(items * rows * cols)), dim3(batch_block), 0, as_stream(s)>>>(
        items, rows, cols, alpha, alpha_cols, b, ldb, x, ldx);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

// out[item, col] = R_W(a[i, col] * b[i, col]) (NORM: its square root, b == a): one workgroup per (item, col)
template <bool NORM, typename T>
__global__ __launch_bounds__(512) void dot_kernel(int64_t rows, int64_t cols, const T* __restrict__ a, int64_t lda,
                                                  const T* __restrict__ b, int64_t ldb, T* __restrict__ out)
{
    __shared__ T red[2 * 512];
    const int w = blockDim.x;
    const int64_t item = blockIdx.x / cols, col = blockIdx.x % cols;
    const T* ai = a + item * rows * lda + col;
    const T* bi = b + item * rows * ldb + col;
    T acc = T(0);
    for (int64_t i = threadIdx.x; i < rows; i += w) acc = acc + ai[i * lda] * bi[i * ldb];
    int half = 0;
    const T r = reduce_w(acc, red, half, w);
    if (threadIdx.x == 0) out[blockIdx.x] = NORM ? sqrt(r) : r;
}

template <bool NORM, typename T>
int dot(gkoc_stream_t s, int64_t items, int64_t rows, int64_t cols, const T* a, int64_t lda, const T* b,
        int64_t ldb, T* out)
{
    GKOC_REQUIRE(items >= 0 && rows >= 0 && cols >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(lda >= cols && ldb >= cols, GKOC_E_INVALID, "a stride smaller than the number of columns");
    GKOC_REQUIRE(items * cols <= INT32_MAX, GKOC_E_INVALID, "more results than one launch holds");
    if (items == 0 || cols == 0) return GKOC_OK;
    GKOC_REQUIRE(out && (rows == 0 || (a && b)), GKOC_E_INVALID, "null pointer");
    dot_kernel<NORM, T><<<dim3(unsigned(items * cols)), dim3(unsigned(batch_width(rows))), 0, as_stream(s)>>>(
        rows, cols, a, lda, b, ldb, out);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

// ------------------------------------------------------------------ values-only conversions
// every slot of every item: the k-th stored entry of row i, 0 beyond the row and in the rows of the padding
template <typename T>
__global__ __launch_bounds__(batch_block) void csr_to_ell_values_kernel(int64_t items, int64_t n_rows, int64_t nnz,
                                                                        const int32_t* __restrict__ rp,
                                                                        int64_t ell_k, int64_t ell_stride,
                                                                        const T* __restrict__ csr_vals,
                                                                        T* __restrict__ ell_vals)
{
    const int64_t per_item = ell_k * ell_stride, total = items * per_item;
    const int64_t step = int64_t(gridDim.x) * batch_block;
    for (int64_t idx = int64_t(blockIdx.x) * batch_block + threadIdx.x; idx < total; idx += step) {
        const int64_t item = idx / per_item, slot = idx - item * per_item;
        const int64_t k = slot / ell_stride, i = slot - k * ell_stride;
        T v = T(0);
        if (i < n_rows) {
            const int64_t begin = rp[i], len = int64_t(rp[i + 1]) - begin;
            if (k < len) v = csr_vals[item * nnz + begin + k];
        }
        ell_vals[idx] = v;
    }
}

// one thread per (item, row): the stored slots of the row in slot order, padding skipped wherever it sits
template <typename T>
__global__ __launch_bounds__(batch_block) void ell_to_csr_values_kernel(int64_t items, int64_t n_rows,
                                                                        int64_t ell_k, int64_t ell_stride,
                                                                        const int32_t* __restrict__ ell_cols,
                                                                        int64_t nnz, const int32_t* __restrict__ rp,
                                                                        const T* __restrict__ ell_vals,
                                                                        T* __restrict__ csr_vals)
{
    const int64_t total = items * n_rows;
    const int64_t step = int64_t(gridDim.x) * batch_block;
    for (int64_t idx = int64_t(blockIdx.x) * batch_block + threadIdx.x; idx < total; idx += step) {
        const int64_t item = idx / n_rows, i = idx - item * n_rows;
        int64_t at = rp[i];
        const int64_t end = rp[i + 1];
        for (int64_t k = 0; k < ell_k && at < end; ++k) {
            if (ell_cols[i + k * ell_stride] >= 0) {
                csr_vals[item * nnz + at] = ell_vals[item * ell_k * ell_stride + i + k * ell_stride];
                ++at;
            }
        }
    }
}

template <typename T>
int csr_to_ell_values(gkoc_stream_t s, int64_t items, int64_t n_rows, int64_t nnz, const int32_t* rp, int64_t ell_k,
                      int64_t ell_stride, const T* csr_vals, T* ell_vals)
{
    GKOC_REQUIRE(items >= 0 && n_rows >= 0 && nnz >= 0 && ell_k >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(ell_stride >= n_rows, GKOC_E_INVALID, "a stride smaller than the number of rows");
    if (items == 0 || ell_k * ell_stride == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && ell_vals && (nnz == 0 || csr_vals), GKOC_E_INVALID, "null pointer");
    csr_to_ell_values_kernel<T><<<dim3(flat_grid(items * ell_k * ell_stride)), dim3(batch_block), 0, as_stream(s)>>>(
        items, n_rows, nnz, rp, ell_k, ell_stride, csr_vals, ell_vals);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

template <typename T>
int ell_to_csr_values(gkoc_stream_t s, int64_t items, int64_t n_rows, int64_t ell_k, int64_t ell_stride,
                      const int32_t* ell_cols, int64_t nnz, const int32_t* rp, const T* ell_vals, T* csr_vals)
{
    GKOC_REQUIRE(items >= 0 && n_rows >= 0 && nnz >= 0 && ell_k >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(ell_stride >= n_rows, GKOC_E_INVALID, "a stride smaller than the number of rows");
    if (items == 0 || n_rows == 0 || nnz == 0) return GKOC_OK;
    GKOC_REQUIRE(rp && csr_vals && ell_cols && ell_vals, GKOC_E_INVALID, "null pointer");
    ell_to_csr_values_kernel<T><<<dim3(flat_grid(items * n_rows)), dim3(batch_block), 0, as_stream(s)>>>(
        items, n_rows, ell_k, ell_stride, ell_cols, nnz, rp, ell_vals, csr_vals);
    GKOC_LAUNCH_OK();
    return GKOC_OK;
}

// ------------------------------------------------------------------ structure checks (set-up; they synchronise)
// flags[0]: row pointers that do not ascend from 0 to nnz, flags[1]: a column outside the matrix
__global__ __launch_bounds__(batch_block) void csr_check_kernel(int64_t n_rows, int64_t n_cols, int64_t nnz,
                                                                const int32_t* __restrict__ rp,
                                                                const int32_t* __restrict__ ci,
                                                                int* __restrict__ flags)
{
    const int64_t step = int64_t(gridDim.x) * batch_block;
    const int64_t first = int64_t(blockIdx.x) * batch_block + threadIdx.x;
    for (int64_t i = first; i <= n_rows; i += step) {
        const int64_t p = rp[i];
        if ((i == 0 && p != 0) || (i == n_rows && p != nnz) || p < 0 || p > nnz ||
            (i < n_rows && int64_t(rp[i + 1]) < p)) {
            flags[0] = 1;
        }
    }
    for (int64_t e = first; e < nnz; e += step) {
        const int64_t c = ci[e];
        if (c < 0 || c >= n_cols) flags[1] = 1;
    }
}

// flags[0]: a slot that is neither -1 nor a column of the matrix
__global__ __launch_bounds__(batch_block) void ell_check_kernel(int64_t n_rows, int64_t n_cols, int64_t ell_k,
                                                                int64_t ell_stride,
                                                                const int32_t* __restrict__ cols,
                                                                int* __restrict__ flags)
{
    const int64_t total = n_rows * ell_k;
    const int64_t step = int64_t(gridDim.x) * batch_block;
    for (int64_t idx = int64_t(blockIdx.x) * batch_block + threadIdx.x; idx < total; idx += step) {
        const int64_t k = idx / n_rows, i = idx - k * n_rows;
        const int64_t c = cols[i + k * ell_stride];
        if (c < -1 || c >= n_cols) flags[0] = 1;
    }
}

int csr_check(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* rp, const int32_t* ci)
{
    GKOC_REQUIRE(n_rows >= 0 && n_cols >= 0 && nnz >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(rp && (nnz == 0 || ci), GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    void* raw = nullptr;
    GKOC_TRY(scratch_malloc(st, &raw, 2 * sizeof(int)));
    scratch_guard guard{st, raw};
    int* flags = static_cast<int*>(raw);
    GKOC_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(int), st));
    const int64_t most = nnz > n_rows + 1 ? nnz : n_rows + 1;
    csr_check_kernel<<<dim3(flat_grid(most)), dim3(batch_block), 0, st>>>(n_rows, n_cols, nnz, rp, ci, flags);
    GKOC_LAUNCH_OK();
    int host[2] = {0, 0};
    GKOC_HIP(hipMemcpyAsync(host, flags, sizeof(host), hipMemcpyDeviceToHost, st));
    GKOC_HIP(hipStreamSynchronize(st));
    GKOC_REQUIRE(host[0] == 0, GKOC_E_INVALID, "row pointers do not ascend from 0 to the number of stored entries");
    GKOC_REQUIRE(host[1] == 0, GKOC_E_INVALID, "a column outside the matrix");
    return GKOC_OK;
}

int ell_check(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, int64_t ell_k, int64_t ell_stride,
              const int32_t* cols)
{
    GKOC_REQUIRE(n_rows >= 0 && n_cols >= 0 && ell_k >= 0, GKOC_E_INVALID, "negative size");
    GKOC_REQUIRE(ell_stride >= n_rows, GKOC_E_INVALID, "a stride smaller than the number of rows");
    if (n_rows * ell_k == 0) return GKOC_OK;
    GKOC_REQUIRE(cols, GKOC_E_INVALID, "null pointer");
    hipStream_t st = as_stream(s);
    void* raw = nullptr;
    GKOC_TRY(scratch_malloc(st, &raw, sizeof(int)));
    scratch_guard guard{st, raw};
    int* flags = static_cast<int*>(raw);
    GKOC_HIP(hipMemsetAsync(flags, 0, sizeof(int), st));
    ell_check_kernel<<<dim3(flat_grid(n_rows * ell_k)), dim3(batch_block), 0, st>>>(n_rows, n_cols, ell_k,
                                                                                   ell_stride, cols, flags);
    GKOC_LAUNCH_OK();
    int host[1] = {0};
    GKOC_HIP(hipMemcpyAsync(host, flags, sizeof(host), hipMemcpyDeviceToHost, st));
    GKOC_HIP(hipStreamSynchronize(st));
    GKOC_REQUIRE(host[0] == 0, GKOC_E_INVALID, "a slot that is neither -1 nor a column of the matrix");
    return GKOC_OK;
}

}  // namespace
}  // namespace gkoc

using namespace gkoc;

extern "C" int gkoc_batch_plan(int solver, int format, int precond, int value_bytes, int64_t n_rows,
                               int64_t stored_per_item, gkoc_batch_plan_info* plan_host)
{
    return make_plan(solver, format, precond, value_bytes, n_rows, stored_per_item, plan_host);
}

extern "C" int gkoc_batch_csr_check_i32(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, int64_t nnz,
                                        const int32_t* row_ptrs, const int32_t* col_idxs)
{
    return csr_check(s, n_rows, n_cols, nnz, row_ptrs, col_idxs);
}

extern "C" int gkoc_batch_ell_check_i32(gkoc_stream_t s, int64_t n_rows, int64_t n_cols, int64_t ell_k,
                                        int64_t ell_stride, const int32_t* ell_cols)
{
    return ell_check(s, n_rows, n_cols, ell_k, ell_stride, ell_cols);
}

#define GKOC_DEF_BATCH_SOLVER(NAME, CODE, T, TN)                                                               \
    extern "C" int gkoc_batch_##NAME##_csr_##TN##_i32(                                                         \
        gkoc_stream_t s, int64_t items, int64_t n_rows, int64_t nnz, const int32_t* row_ptrs,                  \
        const int32_t* col_idxs, const T* vals, int precond, const T* b, int64_t ldb, T* x, int64_t ldx,       \
        double tol, int tol_type, int64_t max_iterations, void* workspace, size_t workspace_bytes,             \
        int* iteration_counts, T* residual_norms, int* converged)                                              \
    {                                                                                                          \
        return solve<CODE, GKOC_BATCH_CSR, T>(s, items, n_rows, nnz, row_ptrs, col_idxs, 0, 0, vals, precond,  \
                                              b, ldb, x, ldx, tol, tol_type, max_iterations, workspace,        \
                                              workspace_bytes, iteration_counts, residual_norms, converged);   \
    }                                                                                                          \
    extern "C" int gkoc_batch_##NAME##_ell_##TN##_i32(                                                         \
        gkoc_stream_t s, int64_t items, int64_t n_rows, int64_t ell_k, int64_t ell_stride,                     \
        const int32_t* ell_cols, const T* vals, int precond, const T* b, int64_t ldb, T* x, int64_t ldx,       \
        double tol, int tol_type, int64_t max_iterations, void* workspace, size_t workspace_bytes,             \
        int* iteration_counts, T* residual_norms, int* converged)                                              \
    {                                                                                                          \
        GKOC_REQUIRE(ell_k >= 0 && ell_stride >= 0, GKOC_E_INVALID, "negative size");                          \
        return solve<CODE, GKOC_BATCH_ELL, T>(s, items, n_rows, ell_k * ell_stride, nullptr, ell_cols, ell_k,  \
                                              ell_stride, vals, precond, b, ldb, x, ldx, tol, tol_type,        \
                                              max_iterations, workspace, workspace_bytes, iteration_counts,    \
                                              residual_norms, converged);                                      \
    }
GKOC_DEF_BATCH_SOLVER(cg, GKOC_BATCH_CG, double, f64)
GKOC_DEF_BATCH_SOLVER(cg, GKOC_BATCH_CG, float, f32)
GKOC_DEF_BATCH_SOLVER(bicgstab, GKOC_BATCH_BICGSTAB, double, f64)
GKOC_DEF_BATCH_SOLVER(bicgstab, GKOC_BATCH_BICGSTAB, float, f32)

#define GKOC_DEF_BATCH(T, TN)                                                                                  \
    extern "C" int gkoc_batch_csr_apply_##TN##_i32(gkoc_stream_t s, int64_t items, int64_t n_rows,             \
                                                   int64_t n_cols, int64_t nnz, const int32_t* row_ptrs,       \
                                                   const int32_t* col_idxs, const T* vals, const T* b,         \
                                                   int64_t ldb, T* x, int64_t ldx, int64_t cols)               \
    {                                                                                                          \
        return apply<GKOC_BATCH_CSR, false, T>(s, items, n_rows, n_cols, nnz, row_ptrs, col_idxs, 0, 0, vals,  \
                                               nullptr, b, ldb, nullptr, x, ldx, cols);                        \
    }                                                                                                          \
    extern "C" int gkoc_batch_csr_advanced_apply_##TN##_i32(                                                   \
        gkoc_stream_t s, int64_t items, int64_t n_rows, int64_t n_cols, int64_t nnz, const T* alpha,           \
        const int32_t* row_ptrs, const int32_t* col_idxs, const T* vals, const T* b, int64_t ldb,              \
        const T* beta, T* x, int64_t ldx, int64_t cols)                                                        \
    {                                                                                                          \
        return apply<GKOC_BATCH_CSR, true, T>(s, items, n_rows, n_cols, nnz, row_ptrs, col_idxs, 0, 0, vals,   \
                                              alpha, b, ldb, beta, x, ldx, cols);                              \
    }                                                                                                          \
    extern "C" int gkoc_batch_ell_apply_##TN##_i32(gkoc_stream_t s, int64_t items, int64_t n_rows,             \
                                                   int64_t n_cols, int64_t ell_k, int64_t ell_stride,          \
                                                   const int32_t* ell_cols, const T* vals, const T* b,         \
                                                   int64_t ldb, T* x, int64_t ldx, int64_t cols)               \
    {                                                                                                          \
        GKOC_REQUIRE(ell_k >= 0 && ell_stride >= 0, GKOC_E_INVALID, "negative size");                          \
        return apply<GKOC_BATCH_ELL, false, T>(s, items, n_rows, n_cols, ell_k * ell_stride, nullptr,          \
                                               ell_cols, ell_k, ell_stride, vals, nullptr, b, ldb, nullptr,    \
                                               x, ldx, cols);                                                  \
    }                                                                                                          \
    extern "C" int gkoc_batch_ell_advanced_apply_##TN##_i32(                                                   \
        gkoc_stream_t s, int64_t items, int64_t n_rows, int64_t n_cols, int64_t ell_k, int64_t ell_stride,     \
        const T* alpha, const int32_t* ell_cols, const T* vals, const T* b, int64_t ldb, const T* beta, T* x,  \
        int64_t ldx, int64_t cols)                                                                             \
    {                                                                                                          \
        GKOC_REQUIRE(ell_k >= 0 && ell_stride >= 0, GKOC_E_INVALID, "negative size");                          \
        return apply<GKOC_BATCH_ELL, true, T>(s, items, n_rows, n_cols, ell_k * ell_stride, nullptr, ell_cols, \
                                              ell_k, ell_stride, vals, alpha, b, ldb, beta, x, ldx, cols);     \
    }                                                                                                          \
    extern "C" int gkoc_batch_scale_##TN(gkoc_stream_t s, int64_t items, int64_t rows, int64_t cols,           \
                                         const T* alpha, int64_t alpha_cols, T* x, int64_t ldx)                \
    {                                                                                                          \
        return scale<false, T>(s, items, rows, cols, alpha, alpha_cols, nullptr, 0, x, ldx);                   \
    }                                                                                                          \
    extern "C" int gkoc_batch_add_scaled_##TN(gkoc_stream_t s, int64_t items, int64_t rows, int64_t cols,      \
                                              const T* alpha, int64_t alpha_cols, const T* b, int64_t ldb,     \
                                              T* x, int64_t ldx)                                               \
    {                                                                                                          \
        return scale<true, T>(s, items, rows, cols, alpha, alpha_cols, b, ldb, x, ldx);                        \
    }                                                                                                          \
    extern "C" int gkoc_batch_compute_dot_##TN(gkoc_stream_t s, int64_t items, int64_t rows, int64_t cols,     \
                                               const T* a, int64_t lda, const T* b, int64_t ldb, T* result)    \
    {                                                                                                          \
        return dot<false, T>(s, items, rows, cols, a, lda, b, ldb, result);                                    \
    }                                                                                                          \
    extern "C" int gkoc_batch_compute_norm2_##TN(gkoc_stream_t s, int64_t items, int64_t rows, int64_t cols,   \
                                                 const T* a, int64_t lda, T* result)                           \
    {                                                                                                          \
        return dot<true, T>(s, items, rows, cols, a, lda, a, lda, result);                                     \
    }                                                                                                          \
    extern "C" int gkoc_batch_csr_to_ell_values_##TN##_i32(gkoc_stream_t s, int64_t items, int64_t n_rows,     \
                                                           int64_t nnz, const int32_t* row_ptrs,               \
                                                           int64_t ell_k, int64_t ell_stride,                  \
                                                           const T* csr_vals, T* ell_vals)                     \
    {                                                                                                          \
        return csr_to_ell_values<T>(s, items, n_rows, nnz, row_ptrs, ell_k, ell_stride, csr_vals, ell_vals);   \
    }                                                                                                          \
    extern "C" int gkoc_batch_ell_to_csr_values_##TN##_i32(gkoc_stream_t s, int64_t items, int64_t n_rows,     \
                                                           int64_t ell_k, int64_t ell_stride,                  \
                                                           const int32_t* ell_cols, int64_t nnz,               \
                                                           const int32_t* row_ptrs, const T* ell_vals,         \
                                                           T* csr_vals)                                        \
    {                                                                                                          \
        return ell_to_csr_values<T>(s, items, n_rows, ell_k, ell_stride, ell_cols, nnz, row_ptrs, ell_vals,    \
                                    csr_vals);                                                                 \
    }
GKOC_DEF_BATCH(double, f64)
GKOC_DEF_BATCH(float, f32)
