// Diagonal Gaussian-mixture head: masked negative log-likelihood, its gradient and the inverse-CDF
// sampler (reference layers.py:157-195, utils/loss.py:111-199, models/simulator.py:13-57; mgn.h).
//
// One thread owns one row. A row is K(2d+1) floats (21 at K = 3, d = 3: 84 bytes, not a multiple of 16)
// and every one of them is used by that thread alone: there is nothing to share through the LDS, and
// consecutive lanes read consecutive rows, so a wave's loads of one column walk one contiguous
// 64·K(2d+1)·4-byte span whose cache lines are all consumed from the vector L1 by the loads of the next
// columns. Staging through the LDS would add a round trip (and a K-dependent padding against bank
// conflicts: the row length is even whenever K is) without saving one byte of HBM traffic; the kernels
// are bound by that traffic and by the exp / log of the row, so rows are read per thread. The component
// loops are unrolled over the supported maximum with a k < K guard: the per-component values stay in
// registers (a runtime-indexed array would live in scratch).
#include "mgn_common.h"

namespace {

constexpr int GMM_MAX_K = 16, GMM_MAX_D = 8;
constexpr int GMM_BLOCKS = 64;  // partial sums of the loss (as MSE_BLOCKS of mgn_masked_mse)
constexpr float GMM_EPS = 1e-12f;
constexpr float GMM_LOG_2PI = 1.8378770664093453f;

// a[k] = softmax(logit)_k, lm[k] = log(a_k + eps) + lc_k; returns L = logsumexp_k lm[k]: the reference's
// expression term for term, in its order of operations.
__device__ __forceinline__ float gmm_row_terms(const float* __restrict__ p, const float* __restrict__ x, int d,
                                               int K, float temperature, float (&a)[GMM_MAX_K],
                                               float (&lm)[GMM_MAX_K]) {
    const int pc = 2 * d + 1;
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < GMM_MAX_K; ++k)
        if (k < K) mx = fmaxf(mx, p[k * pc]);
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < GMM_MAX_K; ++k)
        if (k < K) {
            a[k] = expf(p[k * pc] - mx);
            den += a[k];
        }
    float lmax = -INFINITY;
#pragma unroll
    for (int k = 0; k < GMM_MAX_K; ++k)
        if (k < K) {
            a[k] = a[k] / den;
            const float* q = p + k * pc;
            float lc = 0.f;
            for (int j = 0; j < d; ++j) {
                const float diff = x[j] - q[1 + j];
                const float s = expf(q[1 + d + j]) * temperature;
                const float var = s * s;
                lc += -0.5f * (2.f * logf(s + GMM_EPS) + diff * diff / (var + GMM_EPS) + GMM_LOG_2PI);
            }
            lm[k] = logf(a[k] + GMM_EPS) + lc;
            lmax = fmaxf(lmax, lm[k]);
        }
    const float shift = isinf(lmax) ? 0.f : lmax;  // torch.logsumexp: an infinite maximum is not subtracted
    float se = 0.f;
#pragma unroll
    for (int k = 0; k < GMM_MAX_K; ++k)
        if (k < K) se += expf(lm[k] - shift);
    return shift + logf(se);
}

// partial sums per block (fixed row range, strided threads, LDS tree) -> part[block] = {Σ m·L, Σ m}
__global__ __launch_bounds__(256) void gmm_nll_partial(const float* __restrict__ params,
                                                       const float* __restrict__ tgt, int64_t rows, int d, int K,
                                                       float temperature, const float* __restrict__ nt,
                                                       int64_t nt_ld, unsigned tmask, int64_t rows_per_block,
                                                       float* __restrict__ part) {
    __shared__ float ra[256], rc[256];
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < rows ? r0 + rows_per_block : rows;
    const int P = K * (2 * d + 1);
    float acc = 0.f, cnt = 0.f;
    for (int64_t r = r0 + threadIdx.x; r < r1; r += 256) {
        if (type_mask_of(nt, nt_ld, r, tmask) != 0.f) {
            float a[GMM_MAX_K], lm[GMM_MAX_K];
            acc += gmm_row_terms(params + r * P, tgt + r * d, d, K, temperature, a, lm);
            cnt += 1.f;
        }
    }
    ra[threadIdx.x] = acc;
    rc[threadIdx.x] = cnt;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            ra[threadIdx.x] += ra[threadIdx.x + w];
            rc[threadIdx.x] += rc[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = ra[0];
        part[2 * blockIdx.x + 1] = rc[0];
    }
}

__global__ __launch_bounds__(64) void gmm_nll_final(const float* __restrict__ part, int nblocks,
                                                    const float* count_dev, float* loss, float* count_out) {
    const int lane = threadIdx.x;
    float a = 0.f, c = 0.f;
    for (int b = lane; b < nblocks; b += 64) {
        a += part[2 * b];
        c += part[2 * b + 1];
    }
#pragma unroll
    for (int w = 32; w > 0; w >>= 1) {
        a += __shfl_xor(a, w);
        c += __shfl_xor(c, w);
    }
    if (lane == 0) {
        const float cc = count_dev ? *count_dev : c;
        *loss = cc != 0.f ? -a / cc : 0.f;
        if (count_out) *count_out = cc;
    }
}

__global__ __launch_bounds__(256) void gmm_nll_bwd(const float* __restrict__ params, const float* __restrict__ tgt,
                                                   int64_t rows, int d, int K, float temperature,
                                                   const float* __restrict__ nt, int64_t nt_ld, unsigned tmask,
                                                   const float* count, const float* gout,
                                                   float* __restrict__ grad) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int pc = 2 * d + 1, P = K * pc;
    float* gr = grad + r * P;
    const float c = *count;
    if (c == 0.f || type_mask_of(nt, nt_ld, r, tmask) == 0.f) {
        for (int i = 0; i < P; ++i) gr[i] = 0.f;
        return;
    }
    const float g = -(gout ? *gout : 1.f) / c;
    const float* p = params + r * P;
    const float* x = tgt + r * d;
    float a[GMM_MAX_K], lm[GMM_MAX_K];
    const float L = gmm_row_terms(p, x, d, K, temperature, a, lm);
    float S = 0.f;  // Σ_k r_k a_k / (a_k + eps)
#pragma unroll
    for (int k = 0; k < GMM_MAX_K; ++k)
        if (k < K) {
            const float resp = expf(lm[k] - L);
            const float* q = p + k * pc;
            float* gq = gr + k * pc;
            for (int j = 0; j < d; ++j) {
                const float diff = x[j] - q[1 + j];
                const float s = expf(q[1 + d + j]) * temperature;
                const float var = s * s, den = var + GMM_EPS;
                gq[1 + j] = g * resp * (diff / den);
                gq[1 + d + j] = g * resp * (diff * diff / den * (var / den) - s / (s + GMM_EPS));
            }
            lm[k] = resp * (a[k] / (a[k] + GMM_EPS));
            S += lm[k];
        }
#pragma unroll
    for (int k = 0; k < GMM_MAX_K; ++k)
        if (k < K) gr[k * pc] = g * (lm[k] - a[k] * S);
}

__global__ __launch_bounds__(256) void gmm_sample(const float* __restrict__ params, int64_t rows, int d, int K,
                                                  float temperature, const float* __restrict__ u,
                                                  const float* __restrict__ z, float* __restrict__ out) {
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= rows) return;
    const int pc = 2 * d + 1;
    const float* p = params + r * K * pc;
    float mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < GMM_MAX_K; ++k)
        if (k < K) mx = fmaxf(mx, p[k * pc]);
    float e[GMM_MAX_K];
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < GMM_MAX_K; ++k)
        if (k < K) {
            e[k] = expf(p[k * pc] - mx);
            den += e[k];
        }
    const float ur = u[r];
    float cum = 0.f;
    int sel = K - 1;  // the last component catches what rounding leaves of the running sum
#pragma unroll
    for (int k = 0; k < GMM_MAX_K; ++k)
        if (k < K) {
            cum += e[k] / den;
            if (cum > ur && k < sel) sel = k;
        }
    const float* q = p + sel * pc;
    for (int j = 0; j < d; ++j) out[r * d + j] = q[1 + j] + expf(q[1 + d + j]) * temperature * z[r * d + j];
}

int gmm_check_shape(int32_t d, int32_t K, int64_t rows) {
    MGN_REQUIRE(K >= 1 && K <= GMM_MAX_K, "gmm: the number of mixture components K must be in [1, 16]");
    MGN_REQUIRE(d >= 1 && d <= GMM_MAX_D, "gmm: the output dimension d must be in [1, 8]");
    MGN_REQUIRE(rows >= 0, "gmm: rows must be >= 0");
    return 0;
}

}  // namespace

extern "C" {

size_t mgn_gmm_nll_workspace_bytes(int64_t rows) {
    (void)rows;
    return 2 * GMM_BLOCKS * sizeof(float);
}

int mgn_gmm_nll_diag(const float* params, const float* target, int64_t rows, int32_t d, int32_t K,
                     float temperature, const float* node_type, int64_t nt_ld, uint32_t type_mask,
                     const float* count, float* loss, float* count_out, void* ws, size_t ws_bytes,
                     mgn_stream_t stream) {
    if (int rc = gmm_check_shape(d, K, rows)) return rc;
    MGN_REQUIRE(ws_bytes >= mgn_gmm_nll_workspace_bytes(rows), "gmm_nll_diag: workspace too small");
    hipStream_t st = (hipStream_t)stream;
    float* part = reinterpret_cast<float*>(ws);
    int64_t rpb = cdiv64(rows > 0 ? rows : 1, GMM_BLOCKS);
    if (rpb < 256) rpb = 256;
    const int nb = (int)cdiv64(rows > 0 ? rows : 1, rpb);
    hipLaunchKernelGGL(gmm_nll_partial, dim3(nb), dim3(256), 0, st, params, target, rows, (int)d, (int)K,
                       temperature, node_type, nt_ld, type_mask, rpb, part);
    MGN_LAUNCH_CHECK();
    hipLaunchKernelGGL(gmm_nll_final, dim3(1), dim3(64), 0, st, (const float*)part, nb, count, loss, count_out);
    MGN_LAUNCH_CHECK();
    return 0;
}

int mgn_gmm_nll_diag_backward(const float* params, const float* target, int64_t rows, int32_t d, int32_t K,
                              float temperature, const float* node_type, int64_t nt_ld, uint32_t type_mask,
                              const float* count, const float* grad_loss, float* grad, mgn_stream_t stream) {
    if (int rc = gmm_check_shape(d, K, rows)) return rc;
    MGN_REQUIRE(count != nullptr, "gmm_nll_diag_backward: count (the forward's count_out) is required");
    if (rows == 0) return 0;
    hipLaunchKernelGGL(gmm_nll_bwd, dim3((unsigned)cdiv64(rows, 256)), dim3(256), 0, (hipStream_t)stream, params,
                       target, rows, (int)d, (int)K, temperature, node_type, nt_ld, type_mask, count, grad_loss,
                       grad);
    MGN_LAUNCH_CHECK();
    return 0;
}

int mgn_gmm_sample_diag(const float* params, int64_t rows, int32_t d, int32_t K, float temperature, const float* u,
                        const float* z, float* out, mgn_stream_t stream) {
    if (int rc = gmm_check_shape(d, K, rows)) return rc;
    if (rows == 0) return 0;
    hipLaunchKernelGGL(gmm_sample, dim3((unsigned)cdiv64(rows, 256)), dim3(256), 0, (hipStream_t)stream, params,
                       rows, (int)d, (int)K, temperature, u, z, out);
    MGN_LAUNCH_CHECK();
    return 0;
}

}  // extern "C"
