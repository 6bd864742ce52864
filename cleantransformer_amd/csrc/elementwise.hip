// What is left of the small kernels: error plumbing of the library, activation dropout, embedding, argmax and the decode helpers, mask_prep.
#include "common.h"
#include "prof.h"
#include <hip/amd_detail/amd_hip_unsafe_atomics.h>

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";
void ctmi_set_error(const char* fmt, ...) {
    va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
}
extern "C" const char* ctmi_last_error(void) { return g_err; }
static thread_local bool g_attr_err = false;
void ctmi_dyn_lds(const void* kern, size_t lds_bytes) {
    const hipError_t e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        ctmi_set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize = %zu bytes) refused: %s", lds_bytes, hipGetErrorString(e));
        g_attr_err = true;
    }
}
bool ctmi_take_attr_error() { const bool r = g_attr_err; g_attr_err = false; return r; }
extern "C" int ctmi_abi_version(void) { return CTMI_ABI_VERSION; }

// ------------------------------------------------------------------------------------------------
// activation dropout (hidden / embedding / residual-branch dropout of the reference's modules)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void dropout_k(const T* __restrict__ x, const T* __restrict__ res, T* __restrict__ y, int64_t n,
                                                 uint32_t thr, uint32_t seed, float scale, int vec_ok) {
    constexpr int VEC = 16 / sizeof(T);
    const int64_t nv = vec_ok ? n / VEC : 0;
    for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < nv; v += (int64_t)gridDim.x * 256) {
        float a[VEC], r[VEC];
        unpack16<T>(*reinterpret_cast<const uint4*>(x + v * VEC), a);
        if (res != nullptr) unpack16<T>(*reinterpret_cast<const uint4*>(res + v * VEC), r);
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const bool keep = ctmi_keep_hash((uint32_t)(v * VEC + j), seed) >= thr;
            a[j] = keep ? a[j] * scale : 0.f;
            if (res != nullptr) a[j] += r[j];
        }
        *reinterpret_cast<uint4*>(y + v * VEC) = pack16<T>(a);
    }
    for (int64_t i = nv * VEC + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const bool keep = ctmi_keep_hash((uint32_t)i, seed) >= thr;
        float a = keep ? Cvt<T>::to_f(x[i]) * scale : 0.f;
        if (res != nullptr) a += Cvt<T>::to_f(res[i]);
        y[i] = Cvt<T>::from_f(a);
    }
}
extern "C" uint32_t ctmi_dropout_hash(uint32_t x) { return ctmi_hash32(x); }
extern "C" uint32_t ctmi_dropout_keep_hash(uint32_t counter, uint32_t seed) { return ctmi_keep_hash(counter, seed); }
extern "C" uint32_t ctmi_dropout_threshold(float p) { return ctmi_drop_threshold(p); }
extern "C" int ctmi_dropout(const void* x, const void* residual, void* y, int64_t n, float p, uint32_t seed, int dtype, void* stream) {
    ProfScope prof__(CTMI_PROF_OTHER, as_stream(stream));
    CTMI_REQUIRE(x && y && n >= 0, "dropout: bad args");
    CTMI_REQUIRE(p >= 0.0f && p < 1.0f, "dropout: p must be in [0, 1)");
    if (n == 0) return CTMI_OK;
    const uint32_t thr = ctmi_drop_threshold(p);
    const float scale = 1.0f / (1.0f - p);
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(n, 256 * 8), 8192);
    const int vec_ok = aligned16(x) && aligned16(y) && (residual == nullptr || aligned16(residual));
    return ctmi_by_dtype(dtype, "dropout", [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((dropout_k<T>), dim3(grid), dim3(256), 0, as_stream(stream), (const T*)x, (const T*)residual, (T*)y, n, thr, seed, scale, vec_ok);
        CTMI_CHECK_LAUNCH("dropout");
        return CTMI_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// embedding gather / scatter-add   (modeling_bloom.py:190)
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void embed_fwd_k(const T* __restrict__ table, const int64_t* __restrict__ ids,
                                                   T* __restrict__ out, int64_t n, int64_t H, int64_t V, int vec_ok,
                                                   int32_t* err_flag) {
    constexpr int VEC = 16 / sizeof(T);
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    for (int64_t t = wave0; t < n; t += (int64_t)gridDim.x * 4) {
        int64_t id = ids[t];
        if (id < 0 || id >= V) { if (lane == 0 && err_flag) atomicExch(err_flag, 1); id = 0; }
        const T* src = table + id * H;
        T* dst = out + t * H;
        if (vec_ok) {
            for (int64_t c = (int64_t)lane * VEC; c < H; c += 64 * VEC)
                *reinterpret_cast<uint4*>(dst + c) = *reinterpret_cast<const uint4*>(src + c);
        } else {
            for (int64_t c = lane; c < H; c += 64) dst[c] = src[c];
        }
    }
}
template <typename T>
__global__ __launch_bounds__(256) void embed_bwd_k(const T* __restrict__ dout, const int64_t* __restrict__ ids,
                                                   float* __restrict__ dtable, int64_t n, int64_t H, int64_t V, float scale) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    for (int64_t t = wave0; t < n; t += (int64_t)gridDim.x * 4) {
        const int64_t id = ids[t];
        if (id < 0 || id >= V) continue;
        float* dst = dtable + id * H;
        const T* src = dout + t * H;
        for (int64_t c = lane; c < H; c += 64) unsafeAtomicAdd(dst + c, scale * Cvt<T>::to_f(src[c]));
    }
}

extern "C" int ctmi_embed_fwd(const void* table, const int64_t* ids, void* out, int64_t n, int64_t H, int64_t V,
                              int dtype, int32_t* err_flag, void* stream) {
    ProfScope prof__(CTMI_PROF_OTHER, as_stream(stream));
    CTMI_REQUIRE(table && ids && out && n >= 0 && H > 0 && V > 0, "embed_fwd: bad args");
    if (n == 0) return CTMI_OK;
    int grid = (int)std::min<int64_t>(cdiv64(n, 4), 4096);
    return ctmi_by_dtype(dtype, "embed_fwd", [&](auto t) -> int {
        using T = decltype(t);
        constexpr int VEC = 16 / sizeof(T);
        const int vec_ok = (H % VEC == 0) && aligned16(table) && aligned16(out);
        hipLaunchKernelGGL((embed_fwd_k<T>), dim3(grid), dim3(256), 0, as_stream(stream), (const T*)table, ids, (T*)out, n, H, V, vec_ok, err_flag);
        CTMI_CHECK_LAUNCH("embed_fwd");
        return CTMI_OK;
    });
}
extern "C" int ctmi_embed_bwd(const void* dout, const int64_t* ids, float* dtable, int64_t n, int64_t H, int64_t V,
                              int dtype, float scale, void* stream) {
    ProfScope prof__(CTMI_PROF_OTHER, as_stream(stream));
    CTMI_REQUIRE(dout && ids && dtable && n >= 0 && H > 0 && V > 0, "embed_bwd: bad args");
    if (n == 0) return CTMI_OK;
    int grid = (int)std::min<int64_t>(cdiv64(n, 4), 4096);
    return ctmi_by_dtype(dtype, "embed_bwd", [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((embed_bwd_k<T>), dim3(grid), dim3(256), 0, as_stream(stream), (const T*)dout, ids, dtable, n, H, V, scale);
        CTMI_CHECK_LAUNCH("embed_bwd");
        return CTMI_OK;
    });
}

template <typename T>
__global__ __launch_bounds__(256) void argmax_k(const T* __restrict__ x, int64_t ld, int64_t* __restrict__ out, int64_t cols) {
    const T* r = x + (int64_t)blockIdx.x * ld;
    float best = -INFINITY; int64_t bi = INT64_MAX;
    for (int64_t c = threadIdx.x; c < cols; c += 256) {
        const float v = Cvt<T>::to_f(r[c]);
        if (v > best || bi == INT64_MAX) { best = v; bi = c; }          // strictly greater keeps the first index
    }
    for (int o = 32; o > 0; o >>= 1) {
        const float b2 = __shfl_xor(best, o, 64); const int64_t i2 = __shfl_xor(bi, o, 64);
        if (b2 > best || (b2 == best && i2 < bi)) { best = b2; bi = i2; }
    }
    __shared__ float sb[4]; __shared__ int64_t si[4];
    if ((threadIdx.x & 63) == 0) { sb[threadIdx.x >> 6] = best; si[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k) if (sb[k] > best || (sb[k] == best && si[k] < bi)) { best = sb[k]; bi = si[k]; }
        out[blockIdx.x] = bi;
    }
}
extern "C" int ctmi_argmax(const void* x, int64_t ld, int64_t* out, int64_t rows, int64_t cols, int dtype, void* stream) {
    CTMI_REQUIRE(x && out && rows > 0 && cols > 0 && ld >= cols, "argmax: bad args");
    return ctmi_by_dtype(dtype, "argmax", [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((argmax_k<T>), dim3((unsigned)rows), dim3(256), 0, as_stream(stream), (const T*)x, ld, out, cols);
        CTMI_CHECK_LAUNCH("argmax");
        return CTMI_OK;
    });
}

// ------------------------------------------------------------------------------------------------ decode (beam search, samplers)
// Row statistics of log_softmax (generation_util.py:200): stats[row] = {max, log(sum exp(x - max))}, so that the consumer
// forms (x - max) - logsum exactly as torch.log_softmax does.  One workgroup per row; decode is latency-, not HBM-bound.
template <typename T>
__global__ __launch_bounds__(256) void row_lse_k(const T* __restrict__ x, int64_t ld, float* __restrict__ stats, int64_t cols) {
    const T* r = x + (int64_t)blockIdx.x * ld;
    __shared__ float red[4];
    float m = -INFINITY;
    for (int64_t c = threadIdx.x; c < cols; c += 256) m = fmaxf(m, Cvt<T>::to_f(r[c]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
    for (int64_t c = threadIdx.x; c < cols; c += 256) sum += expf(Cvt<T>::to_f(r[c]) - m);
    sum = wave_sum(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        stats[2 * blockIdx.x] = m;
        stats[2 * blockIdx.x + 1] = logf((red[0] + red[1]) + (red[2] + red[3]));
    }
}
extern "C" int ctmi_row_lse(const void* x, int64_t ld, float* stats, int64_t rows, int64_t cols, int dtype, void* stream) {
    CTMI_REQUIRE(x && stats && rows > 0 && cols > 0 && ld >= cols, "row_lse: bad args");
    return ctmi_by_dtype(dtype, "row_lse", [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((row_lse_k<T>), dim3((unsigned)rows), dim3(256), 0, as_stream(stream), (const T*)x, ld, stats, cols);
        CTMI_CHECK_LAUNCH("row_lse");
        return CTMI_OK;
    });
}

// Top-k over the `group` x cols candidates of one batch element (generation_util.py:199-224: scores.view(bsz, -1).topk(2*beam)):
//     score(i, v) = ((x[g*group + i][v] - max_i) - logsum_i) + add[g*group + i] * add_mul       (stats / add optional)
// Output k (value, flat index i*cols + v) pairs in descending value order, equal values by ascending flat index.
// Selection by k rounds of a lexicographic arg-max over the candidates that come after the previous pick: no per-thread
// candidate lists (dynamic register arrays would live in scratch), exact for -inf entries and duplicates; the candidate set
// (group * cols * 4 B <= a few MiB) stays in L2 between rounds.
template <typename T>
__global__ __launch_bounds__(1024) void group_topk_k(const T* __restrict__ x, int64_t ld, const float* __restrict__ stats,
                                                     const float* __restrict__ add, float add_mul, float* __restrict__ out_val,
                                                     int64_t* __restrict__ out_idx, int group, int64_t cols, int k) {
    const int64_t g = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __shared__ float sv[16]; __shared__ int64_t si[16];
    __shared__ float pick_v; __shared__ int64_t pick_i;
    float pv = INFINITY; int64_t pi = -1;                         // previous pick: everything is "after" it
    for (int r = 0; r < k; ++r) {
        float bv = -INFINITY; int64_t bi = INT64_MAX;
        for (int i = 0; i < group; ++i) {
            const int64_t row = g * group + i;
            const T* xr = x + row * ld;
            const float mx = stats ? stats[2 * row] : 0.f, ls = stats ? stats[2 * row + 1] : 0.f;
            const float a = add ? add[row] * add_mul : 0.f;
            for (int64_t c = tid; c < cols; c += 1024) {
                float v = Cvt<T>::to_f(xr[c]);
                if (stats) v = (v - mx) - ls;
                if (add) v = v + a;
                const int64_t f = (int64_t)i * cols + c;
                const bool after = (v < pv) || (v == pv && f > pi);
                if (after && (v > bv || (v == bv && f < bi))) { bv = v; bi = f; }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(bv, o, 64); const int64_t i2 = __shfl_xor(bi, o, 64);
            if (v2 > bv || (v2 == bv && i2 < bi)) { bv = v2; bi = i2; }
        }
        if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
        __syncthreads();
        if (tid == 0) {
            for (int w = 1; w < 16; ++w) if (sv[w] > bv || (sv[w] == bv && si[w] < bi)) { bv = sv[w]; bi = si[w]; }
            pick_v = bv; pick_i = bi;
            out_val[g * k + r] = bv; out_idx[g * k + r] = bi;
        }
        __syncthreads();
        pv = pick_v; pi = pick_i;
    }
}
extern "C" int ctmi_group_topk(const void* x, int64_t ld, const float* stats, const float* add, float add_mul, float* out_val,
                               int64_t* out_idx, int64_t groups, int group, int64_t cols, int k, int dtype, void* stream) {
    CTMI_REQUIRE(x && out_val && out_idx && groups > 0 && group > 0 && cols > 0 && ld >= cols, "group_topk: bad args");
    CTMI_REQUIRE(k > 0 && (int64_t)k <= (int64_t)group * cols, "group_topk: k must be in [1, group*cols]");
    return ctmi_by_dtype(dtype, "group_topk", [&](auto t) -> int {
        using T = decltype(t);
        hipLaunchKernelGGL((group_topk_k<T>), dim3((unsigned)groups), dim3(1024), 0, as_stream(stream), (const T*)x, ld, stats, add, add_mul, out_val, out_idx, group, cols, k);
        CTMI_CHECK_LAUNCH("group_topk");
        return CTMI_OK;
    });
}

// Sampler filters on fp32 scores (logits_processor.py:35-56): out = x / divisor, then entries strictly below the row's
// threshold (thr[row * thr_stride], optional) are replaced by `fill`.  A true division, as the reference performs.
__global__ __launch_bounds__(256) void scores_filter_k(const float* __restrict__ x, int64_t ld, float divisor, const float* __restrict__ thr,
                                                       int64_t thr_stride, float fill, float* __restrict__ out, int64_t ldo, int64_t cols) {
    const int64_t row = blockIdx.y;
    const float t = thr ? thr[row * thr_stride] : -INFINITY;
    for (int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x; c < cols; c += (int64_t)gridDim.x * 256) {
        float v = x[row * ld + c];
        if (divisor != 1.0f) v = __fdiv_rn(v, divisor);
        out[row * ldo + c] = (thr && v < t) ? fill : v;
    }
}
extern "C" int ctmi_scores_filter(const float* x, int64_t ld, float divisor, const float* thr, int64_t thr_stride, float fill,
                                  float* out, int64_t ldo, int64_t rows, int64_t cols, void* stream) {
    CTMI_REQUIRE(x && out && rows > 0 && rows < 65536 && cols > 0 && ld >= cols && ldo >= cols, "scores_filter: bad args");
    const unsigned gx = (unsigned)std::min<int64_t>(cdiv64(cols, 256), 1024);
    hipLaunchKernelGGL(scores_filter_k, dim3(gx, (unsigned)rows), dim3(256), 0, as_stream(stream), x, ld, divisor, thr, thr_stride, fill,
                       out, ldo, cols);
    CTMI_CHECK_LAUNCH("scores_filter");
    return CTMI_OK;
}

// attention_mask [B,S] -> ALiBi key positions (cumsum(mask)-1)*mask as fp32, validity as int32 (modeling_bloom.py:328,178)
__global__ __launch_bounds__(64) void mask_prep_k(const int64_t* __restrict__ am, float* __restrict__ kpos,
                                                  int32_t* __restrict__ kvalid, int32_t* __restrict__ first_valid, int64_t S) {
    const int64_t b = blockIdx.x;
    const int lane = threadIdx.x;
    int64_t running = 0;
    int64_t first = S;
    for (int64_t base = 0; base < S; base += 64) {
        const int64_t j = base + lane;
        const int64_t mv = (j < S) ? am[b * S + j] : 0;
        int64_t incl = mv;                                       // inclusive wave scan
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) { const int64_t t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
        if (j < S) {
            kpos[b * S + j] = (float)((running + incl - 1) * mv);
            kvalid[b * S + j] = (mv != 0) ? 1 : 0;
            if (mv != 0 && j < first) first = j;
        }
        running += __shfl(incl, 63, 64);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const int64_t t = __shfl_xor(first, o, 64); first = t < first ? t : first; }
    if (lane == 0) first_valid[b] = (int32_t)first;
}
extern "C" int ctmi_mask_prep(const int64_t* am, float* kpos, int32_t* kvalid, int32_t* first_valid, int64_t B, int64_t S, void* stream) {
    ProfScope prof__(CTMI_PROF_OTHER, as_stream(stream));
    CTMI_REQUIRE(am && kpos && kvalid && first_valid && B > 0 && S > 0, "mask_prep: bad args");
    hipLaunchKernelGGL(mask_prep_k, dim3((unsigned)B), dim3(64), 0, as_stream(stream), am, kpos, kvalid, first_valid, S);
    CTMI_CHECK_LAUNCH("mask_prep");
    return CTMI_OK;
}
