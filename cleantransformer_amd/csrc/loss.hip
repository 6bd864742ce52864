// Cross entropy: hard labels (statistics + gradient kernels), the fused one-pass training form, probability targets, ctmi_scale_if.
// gfx950: one workgroup per vocabulary row, 16-byte loads, fp32 statistics, streaming stores of the gradient.
#include "common.h"
#include "prof.h"

// ------------------------------------------------------------------------------------------------
// cross entropy  (modeling_bloom.py:224-230; loss.py:29-49 in its numerically stable form)
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int64_t ce_target(const int64_t* labels, int64_t row, int64_t seq, int64_t shift, int64_t ignore) {
    const int64_t b = row / seq, s = row - b * seq;
    if (s + shift >= seq) return -1;
    const int64_t t = labels[b * seq + s + shift];
    return (t == ignore) ? -1 : t;
}

template <typename T>
__global__ __launch_bounds__(256) void ce_fwd_k(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                float* __restrict__ row_lse, float* __restrict__ row_loss,
                                                int64_t C, int64_t seq, int64_t shift, int64_t ignore, int vec_ok) {
    constexpr int VEC = 16 / sizeof(T);
    const int64_t row = blockIdx.x;
    const T* x = logits + row * ld;
    float m = -INFINITY, s = 0.f;
    if (vec_ok) {
        const int64_t Cv = C - C % VEC;                                 // odd class counts (GPT-2: 50257): vector head + scalar tail
        for (int64_t c = Cv + threadIdx.x; c < C; c += 256) {
            const float v = Cvt<T>::to_f(x[c]);
            const float mn = fmaxf(m, v);
            const float ms = (mn == -INFINITY) ? 0.f : mn;
            s = s * __expf(m - ms) + __expf(v - ms);
            m = mn;
        }
        for (int64_t c = (int64_t)threadIdx.x * VEC; c < Cv; c += 256 * VEC) {
            float v[VEC];
            unpack16<T>(*reinterpret_cast<const uint4*>(x + c), v);
            float vm = v[0];
#pragma unroll
            for (int j = 1; j < VEC; ++j) vm = fmaxf(vm, v[j]);
            const float mn = fmaxf(m, vm);
            const float ms = (mn == -INFINITY) ? 0.f : mn;
            float add = 0.f;
#pragma unroll
            for (int j = 0; j < VEC; ++j) add += __expf(v[j] - ms);
            s = s * __expf(m - ms) + add;
            m = mn;
        }
    } else {
        for (int64_t c = threadIdx.x; c < C; c += 256) {
            const float v = Cvt<T>::to_f(x[c]);
            const float mn = fmaxf(m, v);
            const float ms = (mn == -INFINITY) ? 0.f : mn;
            s = s * __expf(m - ms) + __expf(v - ms);
            m = mn;
        }
    }
    // threads that saw nothing hold (m=-inf, s=0): __expf(-inf - mn) = 0 keeps them neutral as long as mn is finite.  A trip whose classes
    // are all -inf (a masked vocabulary slice) on such a state has mn = -inf: `ms` subtracts 0 there instead (one select per trip), so the
    // entries add __expf(-inf) = 0 and the state stays (-inf, 0) instead of turning into NaN.  A row that is -inf everywhere stays undefined.
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        const float mn = fmaxf(m, m2);
        const float a = (m == -INFINITY) ? 0.f : s * __expf(m - mn);
        const float b = (m2 == -INFINITY) ? 0.f : s2 * __expf(m2 - mn);
        s = a + b; m = mn;
    }
    __shared__ float sm_m[4], sm_s[4];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sm_m[wid] = m; sm_s[wid] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float M = sm_m[0], S = sm_s[0];
        for (int k = 1; k < 4; ++k) {
            const float m2 = sm_m[k], s2 = sm_s[k];
            const float mn = fmaxf(M, m2);
            const float a = (M == -INFINITY) ? 0.f : S * __expf(M - mn);
            const float b = (m2 == -INFINITY) ? 0.f : s2 * __expf(m2 - mn);
            S = a + b; M = mn;
        }
        const float lse = M + logf(S);
        row_lse[row] = lse;
        const int64_t t = ce_target(labels, row, seq, shift, ignore);
        row_loss[row] = (t >= 0 && t < C) ? (lse - Cvt<T>::to_f(x[t])) : -1.0f;     // -1 marks "no loss"
    }
}

// single block: loss_out[0] = sum(valid row_loss)/denom ; loss_out[1] = 1/denom
__global__ __launch_bounds__(1024) void ce_finalize_k(const float* __restrict__ row_loss, float* __restrict__ loss_out,
                                                      int64_t N, int denom_mode, int64_t denom_rows) {
    __shared__ double sm_s[16];
    __shared__ unsigned long long sm_c[16];
    double s = 0.0; unsigned long long cnt = 0;
    for (int64_t r = threadIdx.x; r < N; r += 1024) {
        const float l = row_loss[r];
        if (l >= 0.f) { s += (double)l; cnt += 1; }
    }
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); cnt += __shfl_xor(cnt, o, 64); }
    if ((threadIdx.x & 63) == 0) { sm_s[threadIdx.x >> 6] = s; sm_c[threadIdx.x >> 6] = cnt; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double S = 0.0; unsigned long long Cn = 0;
        for (int k = 0; k < 16; ++k) { S += sm_s[k]; Cn += sm_c[k]; }
        double denom = denom_mode == 0 ? (double)Cn : (denom_mode == 1 ? (double)denom_rows : 1.0);
        loss_out[0] = (float)(S / denom);                   // 0/0 -> NaN exactly as torch's mean over zero rows
        loss_out[1] = (float)(1.0 / denom);
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ce_bwd_k(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                const float* __restrict__ row_lse, const float* __restrict__ loss_out,
                                                const float* __restrict__ gout, T* __restrict__ dlogits, int64_t ldd,
                                                int64_t C, int64_t seq, int64_t shift, int64_t ignore, int vec_ok) {
    constexpr int VEC = 16 / sizeof(T);
    const int64_t row = blockIdx.x;
    const T* x = logits + row * ld;
    T* d = dlogits + row * ldd;
    const int64_t t = ce_target(labels, row, seq, shift, ignore);
    const bool live = (t >= 0 && t < C);
    const float coef = live ? (gout ? gout[0] : 1.0f) * loss_out[1] : 0.f;
    const float lse = row_lse[row];
    if (vec_ok) {
        const int64_t Cv = C - C % VEC;
        for (int64_t c = Cv + threadIdx.x; c < C; c += 256)
            d[c] = Cvt<T>::from_f(live ? (__expf(Cvt<T>::to_f(x[c]) - lse) - ((c == t) ? 1.0f : 0.0f)) * coef : 0.f);
        for (int64_t c = (int64_t)threadIdx.x * VEC; c < Cv; c += 256 * VEC) {
            float o[VEC];
            if (live) {
                float v[VEC];
                unpack16<T>(ldg_stream16(x + c), v);                      // logits: last use
#pragma unroll
                for (int j = 0; j < VEC; ++j) o[j] = (__expf(v[j] - lse) - ((c + j == t) ? 1.0f : 0.0f)) * coef;
            } else {
#pragma unroll
                for (int j = 0; j < VEC; ++j) o[j] = 0.f;
            }
            stg_stream16(d + c, pack16<T>(o));                            // 4.1 GB of dlogits: far beyond any cache
        }
    } else {
        for (int64_t c = threadIdx.x; c < C; c += 256)
            d[c] = Cvt<T>::from_f(live ? (__expf(Cvt<T>::to_f(x[c]) - lse) - ((c == t) ? 1.0f : 0.0f)) * coef : 0.f);
    }
}

extern "C" int ctmi_ce_fwd(const void* logits, int64_t ld, const int64_t* labels, float* row_lse, float* row_loss,
                           float* loss_out, int64_t N, int64_t C, int64_t seq, int64_t shift, int64_t ignore_index,
                           int denom_mode, int64_t denom_rows, int dtype, void* stream) {
    ProfScope prof__(CTMI_PROF_LOSS, as_stream(stream));
    CTMI_REQUIRE(logits && labels && row_lse && row_loss && loss_out, "ce_fwd: null pointer");
    CTMI_REQUIRE(N > 0 && C > 0 && seq > 0 && N % seq == 0 && shift >= 0 && ld >= C, "ce_fwd: bad shape N=%lld C=%lld seq=%lld", (long long)N, (long long)C, (long long)seq);
    hipStream_t st = as_stream(stream);
    return ctmi_by_dtype(dtype, "ce_fwd", [&](auto t) -> int {
        using T = decltype(t);
        constexpr int VEC = 16 / sizeof(T);
        const int vec_ok = (ld % VEC == 0) && aligned16(logits);
        hipLaunchKernelGGL((ce_fwd_k<T>), dim3((unsigned)N), dim3(256), 0, st, (const T*)logits, ld, labels, row_lse, row_loss, C, seq, shift, ignore_index, vec_ok);
        CTMI_CHECK_LAUNCH("ce_fwd");
        hipLaunchKernelGGL(ce_finalize_k, dim3(1), dim3(1024), 0, st, row_loss, loss_out, N, denom_mode, denom_rows);
        CTMI_CHECK_LAUNCH("ce_finalize");
        return CTMI_OK;
    });
}

extern "C" int ctmi_ce_bwd(const void* logits, int64_t ld, const int64_t* labels, const float* row_lse, const float* loss_out,
                           const float* gout, void* dlogits, int64_t ldd, int64_t N, int64_t C, int64_t seq, int64_t shift,
                           int64_t ignore_index, int dtype, void* stream) {
    ProfScope prof__(CTMI_PROF_LOSS, as_stream(stream));
    CTMI_REQUIRE(logits && labels && row_lse && loss_out && dlogits, "ce_bwd: null pointer");
    CTMI_REQUIRE(N > 0 && C > 0 && seq > 0 && N % seq == 0 && ld >= C && ldd >= C, "ce_bwd: bad shape");
    hipStream_t st = as_stream(stream);
    return ctmi_by_dtype(dtype, "ce_bwd", [&](auto t) -> int {
        using T = decltype(t);
        constexpr int VEC = 16 / sizeof(T);
        const int vec_ok = (ld % VEC == 0) && (ldd % VEC == 0) && aligned16(logits) && aligned16(dlogits);
        hipLaunchKernelGGL((ce_bwd_k<T>), dim3((unsigned)N), dim3(256), 0, st, (const T*)logits, ld, labels, row_lse, loss_out, gout, (T*)dlogits, ldd, C, seq, shift, ignore_index, vec_ok);
        CTMI_CHECK_LAUNCH("ce_bwd");
        return CTMI_OK;
    });
}

// ---- training path: loss AND its gradient in one pass over the logits (modeling_bloom.py:224-230 followed by loss.backward()).
// The two-kernel form reads the 4.1 GB of bf16 logits twice from HBM (statistics, then gradient).  Here ONE 1024-thread
// workgroup owns a row: pass 1 streams the row (502 KB at V = 250880) and forms its log-sum-exp, pass 2 walks the SAME row
// back to front — the most recently fetched lines first — and writes dlogits.  One workgroup per CU (the dynamic LDS request
// enforces it) keeps 256 rows = 128 MiB in flight, inside the 256 MiB Infinity Cache, so the second read does not go to HBM.
// The gradient is written for an upstream gradient of 1 (loss.backward()); ctmi_scale_if rescales it in the rare other case.
// 1/denom is needed before any row is finished, so it is counted from the labels alone by ce_count_k first.
__global__ __launch_bounds__(1024) void ce_count_k(const int64_t* __restrict__ labels, float* __restrict__ loss_out, int64_t N, int64_t C,
                                                   int64_t seq, int64_t shift, int64_t ignore, int denom_mode, int64_t denom_rows) {
    __shared__ unsigned long long sm_c[16];
    unsigned long long cnt = 0;
    for (int64_t r = threadIdx.x; r < N; r += 1024) {
        const int64_t t = ce_target(labels, r, seq, shift, ignore);
        cnt += (t >= 0 && t < C) ? 1 : 0;
    }
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
    if ((threadIdx.x & 63) == 0) sm_c[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long Cn = 0;
        for (int k = 0; k < 16; ++k) Cn += sm_c[k];
        const double denom = denom_mode == 0 ? (double)Cn : (denom_mode == 1 ? (double)denom_rows : 1.0);
        loss_out[1] = (float)(1.0 / denom);
    }
}

template <typename T>
__global__ __launch_bounds__(1024) void ce_fused_k(const T* __restrict__ logits, int64_t ld, const int64_t* __restrict__ labels,
                                                   float* __restrict__ row_lse, float* __restrict__ row_loss,
                                                   const float* __restrict__ loss_out, T* __restrict__ dlogits, int64_t ldd,
                                                   int64_t C, int64_t seq, int64_t shift, int64_t ignore,
                                                   float gfac, const float* __restrict__ gdev) {
    constexpr int VEC = 16 / sizeof(T);
    constexpr int NT = 1024, UNR = 4;
    __shared__ float sm_m[16], sm_s[16];
    const int64_t row = blockIdx.x;
    const T* x = logits + row * ld;
    T* d = dlogits + row * ldd;
    const int64_t Cv = C - C % VEC;                                     // vector body (rows are 16-byte aligned: checked by the host)
    const int64_t nvec = Cv / VEC;                                      // 16-byte chunks in the row
    float m = -INFINITY, s = 0.f;
    // ---- pass 1: online (max, sum exp), UNR independent 16-byte loads in flight per lane
    for (int64_t c = Cv + threadIdx.x; c < C; c += NT) {
        const float v = Cvt<T>::to_f(x[c]);
        const float mn = fmaxf(m, v);
        const float ms = (mn == -INFINITY) ? 0.f : mn;
        s = s * __expf(m - ms) + __expf(v - ms);
        m = mn;
    }
    int64_t i = threadIdx.x;
    for (; i + (UNR - 1) * NT < nvec; i += UNR * NT) {
        uint4 raw[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) raw[u] = *reinterpret_cast<const uint4*>(x + (i + u * NT) * VEC);
        float vm = -INFINITY;
        float v[UNR][VEC];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            unpack16<T>(raw[u], v[u]);
#pragma unroll
            for (int j = 0; j < VEC; ++j) vm = fmaxf(vm, v[u][j]);
        }
        const float mn = fmaxf(m, vm);
        const float ms = (mn == -INFINITY) ? 0.f : mn;
        float add = 0.f;
#pragma unroll
        for (int u = 0; u < UNR; ++u)
#pragma unroll
            for (int j = 0; j < VEC; ++j) add += __expf(v[u][j] - ms);
        s = s * __expf(m - ms) + add;
        m = mn;
    }
    for (; i < nvec; i += NT) {
        float v[VEC];
        unpack16<T>(*reinterpret_cast<const uint4*>(x + i * VEC), v);
        float vm = v[0];
#pragma unroll
        for (int j = 1; j < VEC; ++j) vm = fmaxf(vm, v[j]);
        const float mn = fmaxf(m, vm);
        const float ms = (mn == -INFINITY) ? 0.f : mn;
        float add = 0.f;
#pragma unroll
        for (int j = 0; j < VEC; ++j) add += __expf(v[j] - ms);
        s = s * __expf(m - ms) + add;
        m = mn;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
        const float mn = fmaxf(m, m2);
        const float a = (m == -INFINITY) ? 0.f : s * __expf(m - mn);
        const float b = (m2 == -INFINITY) ? 0.f : s2 * __expf(m2 - mn);
        s = a + b; m = mn;
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { sm_m[wid] = m; sm_s[wid] = s; }
    __syncthreads();
    float M = sm_m[0], S = sm_s[0];                                     // every thread folds the 16 wave states in the same order
#pragma unroll
    for (int k = 1; k < 16; ++k) {
        const float m2 = sm_m[k], s2 = sm_s[k];
        const float mn = fmaxf(M, m2);
        const float a = (M == -INFINITY) ? 0.f : S * __expf(M - mn);
        const float b = (m2 == -INFINITY) ? 0.f : s2 * __expf(m2 - mn);
        S = a + b; M = mn;
    }
    const float lse = M + logf(S);
    const int64_t t = ce_target(labels, row, seq, shift, ignore);
    const bool live = (t >= 0 && t < C);
    if (threadIdx.x == 0) {
        row_lse[row] = lse;
        row_loss[row] = live ? (lse - Cvt<T>::to_f(x[t])) : -1.0f;       // -1 marks "no loss"
    }
    // ---- pass 2: gradient, back to front (the tail of the row is the freshest in the caches)
    // the upstream gradient the caller EXPECTS (1/accumulation steps, a loss scale: gfac * gdev[0]) is folded in here, in fp32, before the one
    // rounding to the storage type; the backward then rescales only if the actual upstream gradient differs (ctmi_scale_if)
    const float coef = live ? loss_out[1] * (gdev != nullptr ? gfac * gdev[0] : gfac) : 0.f;
    for (int64_t c = Cv + threadIdx.x; c < C; c += NT)
        d[c] = Cvt<T>::from_f(live ? (__expf(Cvt<T>::to_f(x[c]) - lse) - ((c == t) ? 1.0f : 0.0f)) * coef : 0.f);
    if (!live) {
        const uint4 z = make_uint4(0u, 0u, 0u, 0u);
        for (int64_t k = threadIdx.x; k < nvec; k += NT) stg_stream16(d + k * VEC, z);
        return;
    }
    int64_t k = nvec - 1 - threadIdx.x;
    for (; k - (UNR - 1) * NT >= 0; k -= UNR * NT) {
        uint4 raw[UNR];
#pragma unroll
        for (int u = 0; u < UNR; ++u) raw[u] = ldg_stream16(x + (k - u * NT) * VEC);       // logits: last use
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
            const int64_t c = (k - u * NT) * VEC;
            float v[VEC], o[VEC];
            unpack16<T>(raw[u], v);
#pragma unroll
            for (int j = 0; j < VEC; ++j) o[j] = (__expf(v[j] - lse) - ((c + j == t) ? 1.0f : 0.0f)) * coef;
            stg_stream16(d + c, pack16<T>(o));
        }
    }
    for (; k >= 0; k -= NT) {
        const int64_t c = k * VEC;
        float v[VEC], o[VEC];
        unpack16<T>(ldg_stream16(x + c), v);
#pragma unroll
        for (int j = 0; j < VEC; ++j) o[j] = (__expf(v[j] - lse) - ((c + j == t) ? 1.0f : 0.0f)) * coef;
        stg_stream16(d + c, pack16<T>(o));
    }
}

extern "C" int ctmi_ce_fwd_bwd(const void* logits, int64_t ld, const int64_t* labels, float* row_lse, float* row_loss,
                               float* loss_out, void* dlogits, int64_t ldd, int64_t N, int64_t C, int64_t seq, int64_t shift,
                               int64_t ignore_index, int denom_mode, int64_t denom_rows, float grad_factor, const float* grad_factor_dev,
                               int dtype, void* stream) {
    ProfScope prof__(CTMI_PROF_LOSS, as_stream(stream));
    CTMI_REQUIRE(logits && labels && row_lse && row_loss && loss_out && dlogits, "ce_fwd_bwd: null pointer");
    CTMI_REQUIRE(N > 0 && C > 0 && seq > 0 && N % seq == 0 && shift >= 0 && ld >= C && ldd >= C, "ce_fwd_bwd: bad shape N=%lld C=%lld seq=%lld", (long long)N, (long long)C, (long long)seq);
    CTMI_REQUIRE(dtype == CTMI_F32 || dtype == CTMI_BF16 || dtype == CTMI_F16, "ce_fwd_bwd: unsupported dtype %d", dtype);
    return ctmi_by_dtype(dtype, "ce_fwd_bwd", [&](auto t) -> int {
        using T = decltype(t);
        constexpr int VEC = 16 / sizeof(T);
        CTMI_REQUIRE(ld % VEC == 0 && ldd % VEC == 0 && aligned16(logits) && aligned16(dlogits),
                     "ce_fwd_bwd: rows must be 16-byte aligned (use ctmi_ce_fwd + ctmi_ce_bwd otherwise)");
        hipStream_t st = as_stream(stream);
        hipLaunchKernelGGL(ce_count_k, dim3(1), dim3(1024), 0, st, labels, loss_out, N, C, seq, shift, ignore_index, denom_mode, denom_rows);
        CTMI_CHECK_LAUNCH("ce_count");
        const size_t lds_hold = 96 * 1024;                               // one workgroup per CU: 256 rows in flight (see above)
        auto kern = &ce_fused_k<T>;
        ctmi_dyn_lds(reinterpret_cast<const void*>(kern), lds_hold);
        hipLaunchKernelGGL(kern, dim3((unsigned)N), dim3(1024), lds_hold, st, (const T*)logits, ld, labels, row_lse, row_loss, loss_out, (T*)dlogits, ldd, C, seq, shift, ignore_index, grad_factor, grad_factor_dev);
        CTMI_CHECK_LAUNCH("ce_fused");
        hipLaunchKernelGGL(ce_finalize_k, dim3(1), dim3(1024), 0, st, row_loss, loss_out, N, denom_mode, denom_rows);
        CTMI_CHECK_LAUNCH("ce_finalize");
        return CTMI_OK;
    });
}

// x *= s[0] / (applied * applied_dev[0]) unless that ratio is exactly 1 (then every workgroup returns after two scalar loads): the backward of
// the fused loss, whose gradient was written for the EXPECTED upstream gradient applied * applied_dev[0] (ctmi_ce_fwd_bwd's grad_factor pair;
// 1 by default).  g_scale_if_passes counts the calls that really rescaled (tests assert "no second pass over [T,V]" with it).
static __device__ unsigned long long g_scale_if_passes;
template <typename T>
__global__ __launch_bounds__(256) void scale_if_k(T* __restrict__ x, int64_t ld, int64_t rows, int64_t cols, const float* __restrict__ sp,
                                                  float applied, const float* __restrict__ applied_dev) {
    const float want = sp[0], have = applied_dev != nullptr ? applied * applied_dev[0] : applied;
    if (want == have) return;
    const float s = want / have;
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&g_scale_if_passes, 1ULL);
    for (int64_t r = blockIdx.x; r < rows; r += gridDim.x)
        for (int64_t c = threadIdx.x; c < cols; c += 256) x[r * ld + c] = Cvt<T>::from_f(Cvt<T>::to_f(x[r * ld + c]) * s);
}
extern "C" int ctmi_scale_if(void* x, int64_t ld, int64_t rows, int64_t cols, const float* s_dev, float applied, const float* applied_dev,
                             int dtype, void* stream) {
    ProfScope prof__(CTMI_PROF_LOSS, as_stream(stream));
    CTMI_REQUIRE(x && s_dev && rows > 0 && cols > 0 && ld >= cols, "scale_if: bad args");
    CTMI_REQUIRE(applied != 0.f, "scale_if: the factor already applied must not be 0");
    const unsigned grid = (unsigned)std::min<int64_t>(rows, 4096);
    return ctmi_by_dtype(dtype, "scale_if", [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((scale_if_k<T>), dim3(grid), dim3(256), 0, as_stream(stream), (T*)x, ld, rows, cols, s_dev, applied, applied_dev);
        CTMI_CHECK_LAUNCH("scale_if");
        return CTMI_OK;
    });
}
extern "C" int64_t ctmi_scale_if_passes(void) {
    unsigned long long v = 0;
    if (hipMemcpyFromSymbol(&v, HIP_SYMBOL(g_scale_if_passes), sizeof(v), 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    return (int64_t)v;
}

// ---- probability targets (the second branch of loss.py:43-46): loss = -sum_{n,c} t[n,c] * log_softmax(x)[n,c]
//      = sum_n ( lse_n * sum_c t[n,c] - sum_c t[n,c] x[n,c] );   dx[n,c] = (softmax[n,c] * sum_c t[n,c] - t[n,c]) * g / denom.
// One workgroup per row, fp32 statistics; the row sums of t are kept for the backward.  Not on the SFT path (general widths,
// scalar loads): the kernels exist so that the module is complete, not to be fast.
template <typename T>
__global__ __launch_bounds__(256) void ce_soft_fwd_k(const T* __restrict__ logits, int64_t ld, const float* __restrict__ target, int64_t ldt,
                                                     float* __restrict__ row_lse, float* __restrict__ row_tsum,
                                                     float* __restrict__ row_loss, int64_t C) {
    const int64_t row = blockIdx.x;
    const T* x = logits + row * ld;
    const float* t = target + row * ldt;
    float m = -INFINITY;
    for (int64_t c = threadIdx.x; c < C; c += 256) m = fmaxf(m, Cvt<T>::to_f(x[c]));
    __shared__ float red[3][4];
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[0][threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0][0], red[0][1]), fmaxf(red[0][2], red[0][3]));
    __syncthreads();
    float s = 0.f, ts = 0.f, tx = 0.f;
    for (int64_t c = threadIdx.x; c < C; c += 256) {
        const float v = Cvt<T>::to_f(x[c]), tv = t[c];
        s += expf(v - m); ts += tv; tx += tv * v;
    }
    s = wave_sum(s); ts = wave_sum(ts); tx = wave_sum(tx);
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = s; red[1][threadIdx.x >> 6] = ts; red[2][threadIdx.x >> 6] = tx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const float S = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
        const float TS = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
        const float TX = (red[2][0] + red[2][1]) + (red[2][2] + red[2][3]);
        const float lse = m + logf(S);
        row_lse[row] = lse; row_tsum[row] = TS; row_loss[row] = lse * TS - TX;
    }
}
// single block: loss_out[0] = sum(row_loss)/denom over ALL rows (a soft-target row loss may be negative), loss_out[1] = 1/denom
__global__ __launch_bounds__(1024) void ce_soft_finalize_k(const float* __restrict__ row_loss, float* __restrict__ loss_out, int64_t N, double denom) {
    __shared__ double sm_s[16];
    double s = 0.0;
    for (int64_t r = threadIdx.x; r < N; r += 1024) s += (double)row_loss[r];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) sm_s[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double S = 0.0;
        for (int k = 0; k < 16; ++k) S += sm_s[k];
        loss_out[0] = (float)(S / denom); loss_out[1] = (float)(1.0 / denom);
    }
}
template <typename T>
__global__ __launch_bounds__(256) void ce_soft_bwd_k(const T* __restrict__ logits, int64_t ld, const float* __restrict__ target, int64_t ldt,
                                                     const float* __restrict__ row_lse, const float* __restrict__ row_tsum,
                                                     const float* __restrict__ loss_out, const float* __restrict__ gout,
                                                     T* __restrict__ dlogits, int64_t ldd, int64_t C) {
    const int64_t row = blockIdx.x;
    const float coef = (gout ? gout[0] : 1.0f) * loss_out[1], lse = row_lse[row], ts = row_tsum[row];
    for (int64_t c = threadIdx.x; c < C; c += 256)
        dlogits[row * ldd + c] = Cvt<T>::from_f((expf(Cvt<T>::to_f(logits[row * ld + c]) - lse) * ts - target[row * ldt + c]) * coef);
}
extern "C" int ctmi_ce_soft_fwd(const void* logits, int64_t ld, const float* target, int64_t ldt, float* row_lse, float* row_tsum,
                                float* row_loss, float* loss_out, int64_t N, int64_t C, int denom_mode, int64_t denom_rows, int dtype,
                                void* stream) {
    ProfScope prof__(CTMI_PROF_LOSS, as_stream(stream));
    CTMI_REQUIRE(logits && target && row_lse && row_tsum && row_loss && loss_out, "ce_soft_fwd: null pointer");
    CTMI_REQUIRE(N > 0 && C > 0 && ld >= C && ldt >= C && (denom_mode == 1 || denom_mode == 2), "ce_soft_fwd: bad args");
    hipStream_t st = as_stream(stream);
    return ctmi_by_dtype(dtype, "ce_soft_fwd", [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((ce_soft_fwd_k<T>), dim3((unsigned)N), dim3(256), 0, st, (const T*)logits, ld, target, ldt, row_lse, row_tsum, row_loss, C);
        CTMI_CHECK_LAUNCH("ce_soft_fwd");
        hipLaunchKernelGGL(ce_soft_finalize_k, dim3(1), dim3(1024), 0, st, row_loss, loss_out, N, denom_mode == 1 ? (double)denom_rows : 1.0);
        CTMI_CHECK_LAUNCH("ce_soft_finalize");
        return CTMI_OK;
    });
}
extern "C" int ctmi_ce_soft_bwd(const void* logits, int64_t ld, const float* target, int64_t ldt, const float* row_lse,
                                const float* row_tsum, const float* loss_out, const float* gout, void* dlogits, int64_t ldd,
                                int64_t N, int64_t C, int dtype, void* stream) {
    ProfScope prof__(CTMI_PROF_LOSS, as_stream(stream));
    CTMI_REQUIRE(logits && target && row_lse && row_tsum && loss_out && dlogits, "ce_soft_bwd: null pointer");
    CTMI_REQUIRE(N > 0 && C > 0 && ld >= C && ldt >= C && ldd >= C, "ce_soft_bwd: bad shape");
    hipStream_t st = as_stream(stream);
    return ctmi_by_dtype(dtype, "ce_soft_bwd", [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((ce_soft_bwd_k<T>), dim3((unsigned)N), dim3(256), 0, st, (const T*)logits, ld, target, ldt, row_lse, row_tsum, loss_out, gout, (T*)dlogits, ldd, C);
        CTMI_CHECK_LAUNCH("ce_soft_bwd");
        return CTMI_OK;
    });
}
