// Low-rank adapter (LoRA) products for gfx950: three families whose small dimension r is 8..64, where the 128/256-wide GEMM tiles of gemm.hip
// would compute mostly padding.  All three are one pass over the large operand, fp32 accumulation on v_mfma_f32_16x16x32 (bf16 / f16).
//
//   project     out[T,r]  = alpha * X[T,K] W^T          W [r,K] or k-major [K,r]            reads T*K*2 bytes
//   expand-add  Y[T,N]   += Xa[T,r] W                   W [N,r] or [r,N]; in place           moves 2*T*N*2 bytes
//   wgrad       out[P,Q]  = alpha * L[T,P]^T R[T,Q]     fp32 out; T split into slabs that a second launch adds in slab order (no atomics)
//
// Extents: any T >= 1; K, N, P, Q, r and every leading dimension a multiple of 8 (16-byte rows), 8 <= r <= 64, 16-byte aligned pointers.  Every
// 16-byte access covers 8 consecutive elements of one row, so with extents that are multiples of 8 a piece is wholly inside or wholly outside:
// ragged edges are predicated per piece (rows >= T, columns >= the extent are neither read nor written).
#include "mma.h"

namespace {

template <typename T> __device__ __forceinline__ short8 ld_frag(const T* p, bool ok) {
    short8 z = {0, 0, 0, 0, 0, 0, 0, 0};
    return ok ? *reinterpret_cast<const short8*>(p) : z;
}
// 8 elements of one column (stride `ld` between them): the k-major operand layouts
template <typename T> __device__ __forceinline__ short8 ld_frag_strided(const T* p, int64_t ld, bool ok) {
    short8 f = {0, 0, 0, 0, 0, 0, 0, 0};
    if (ok) {
        const uint16_t* q = reinterpret_cast<const uint16_t*>(p);
#pragma unroll
        for (int i = 0; i < 8; ++i) f[i] = (short)q[i * ld];
    }
    return f;
}

// ---------------------------------------------------------------- project
// One workgroup = 16 rows of X; its four waves take the 64-wide K chunks c = wave, wave + 4, ... (one 128-byte line per row and chunk) and their
// partial 16 x r products are added in wave order through LDS.  T / 16 workgroups: 512 at T = 8192, two per CU.
template <typename T, int NT, bool KMAJOR>
__global__ __launch_bounds__(256) void lora_project_k(const T* __restrict__ X, int64_t ldx, const T* __restrict__ W, int64_t ldw, T* __restrict__ out,
                                                       int64_t ldo, int64_t Trows, int K, int r, float alpha) {
    __shared__ float part[4][NT][4][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int64_t t0 = (int64_t)blockIdx.x * 16;
    const int64_t row = t0 + m;
    const bool row_ok = row < Trows;
    const T* xrow = X + (row_ok ? row : 0) * ldx;
    f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int kc = wave * 64; kc < K; kc += 256) {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const int k = kc + s * 32 + g * 8;
            const bool k_ok = k < K;
            const short8 a = ld_frag(xrow + k, row_ok && k_ok);
#pragma unroll
            for (int j = 0; j < NT; ++j) {
                const int n = j * 16 + m;
                const bool ok = k_ok && n < r;
                const short8 b = KMAJOR ? ld_frag_strided(W + (int64_t)(ok ? k : 0) * ldw + (ok ? n : 0), ldw, ok)
                                        : ld_frag(W + (int64_t)(ok ? n : 0) * ldw + (ok ? k : 0), ok);
                acc[j] = Mma<T>::mma(a, b, acc[j]);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) part[wave][j][i][lane] = acc[j][i];
    __syncthreads();
    if (wave < NT) {
        const int n = wave * 16 + m;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float v = ((part[0][wave][i][lane] + part[1][wave][i][lane]) + part[2][wave][i][lane]) + part[3][wave][i][lane];
            const int64_t t = t0 + g * 4 + i;
            if (t < Trows && n < r) out[t * ldo + n] = Cvt<T>::from_f(alpha * v);
        }
    }
}

// ---------------------------------------------------------------- expand-add
// The product is formed transposed (W rows on the MFMA's row side, Xa rows on its column side), with the 16 MFMA rows of a tile mapped to columns
// n = nb + (m >> 2) * 8 + (m & 3) (+ 4 for the second tile of a pair): a lane then holds 8 CONSECUTIVE columns of one row of Y, i.e. one 16-byte
// read-modify-write.  A wave owns 64 columns (four tiles; the W fragments are loaded once, whichever layout W has) and walks 128 rows.
#define LORA_EXP_ROWS 128
template <typename T, int KS, bool KMAJOR>
__global__ __launch_bounds__(256) void lora_expand_add_k(const T* __restrict__ Xa, int64_t ldxa, const T* __restrict__ W, int64_t ldw, T* __restrict__ Y,
                                                          int64_t ldy, int64_t Trows, int N, int r) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int nb = (blockIdx.x * 4 + wave) * 64;
    if (nb >= N) return;
    short8 wf[4][KS];
#pragma unroll
    for (int q = 0; q < 4; ++q) {                            // tile q: pair q >> 1 (32 columns), half q & 1
        const int n = nb + (q >> 1) * 32 + (m >> 2) * 8 + (q & 1) * 4 + (m & 3);
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = s * 32 + g * 8;
            const bool ok = n < N && k < r;
            wf[q][s] = KMAJOR ? ld_frag_strided(W + (int64_t)(ok ? k : 0) * ldw + (ok ? n : 0), ldw, ok)
                              : ld_frag(W + (int64_t)(ok ? n : 0) * ldw + (ok ? k : 0), ok);
        }
    }
    const int64_t tb = (int64_t)blockIdx.y * LORA_EXP_ROWS;
    for (int it = 0; it < LORA_EXP_ROWS / 16; ++it) {
        const int64_t t = tb + it * 16 + m;
        if (tb + it * 16 >= Trows) break;
        const bool row_ok = t < Trows;
        short8 xf[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int k = s * 32 + g * 8;
            xf[s] = ld_frag(Xa + (row_ok ? t : 0) * ldxa + (k < r ? k : 0), row_ok && k < r);
        }
        uint4 old[2];
        bool ok[2];
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int n = nb + p * 32 + g * 8;
            ok[p] = row_ok && n < N;
            old[p] = ok[p] ? *reinterpret_cast<const uint4*>(Y + t * ldy + n) : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            f32x4 lo = {0.f, 0.f, 0.f, 0.f}, hi = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                lo = Mma<T>::mma(wf[p * 2][s], xf[s], lo);
                hi = Mma<T>::mma(wf[p * 2 + 1][s], xf[s], hi);
            }
            float v[8];
            unpack16<T>(old[p], v);
#pragma unroll
            for (int i = 0; i < 4; ++i) { v[i] += lo[i]; v[4 + i] += hi[i]; }
            if (ok[p]) st_wt16(Y + t * ldy + nb + p * 32 + g * 8, pack16<T>(v));
        }
    }
}

// ---------------------------------------------------------------- skinny weight gradient
// out tile 64 x 64 (P x Q) per workgroup; T is cut into `splits` slabs of `chunk` 64-row stages.  A stage's [64 t, 64] pieces of L and R are brought
// into LDS with 16-byte loads (the next stage's are in registers while this one is multiplied) and the fragments — 8 consecutive t of one column —
// are read back transposed.  The live 16 x 16 sub-tiles (at most 16; 4 when min(P, Q) = 16) are dealt round-robin to the four waves.
#define LORA_WG_LD 72                                         // 64 + 8 elements: rows stay 16-byte aligned
template <typename T>
__global__ __launch_bounds__(256) void lora_wgrad_k(const T* __restrict__ L, int64_t ldl, const T* __restrict__ R, int64_t ldr, float* __restrict__ ws,
                                                     int64_t Trows, int P, int Q, int qtiles, int chunk) {
    __shared__ __attribute__((aligned(16))) uint16_t sL[64 * LORA_WG_LD];
    __shared__ __attribute__((aligned(16))) uint16_t sR[64 * LORA_WG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m = lane & 15, g = lane >> 4;
    const int p0 = (blockIdx.x / qtiles) * 64, q0 = (blockIdx.x % qtiles) * 64;
    const int PT = min(4, (P - p0 + 15) / 16), QT = min(4, (Q - q0 + 15) / 16);
    const int64_t tbeg = (int64_t)blockIdx.y * chunk * 64;
    const int64_t tend = min(Trows, tbeg + (int64_t)chunk * 64);
    // this thread's two 16-byte pieces of each operand per stage: rows lr and lr + 32, columns lc .. lc + 7
    const int lr = tid >> 3, lc = (tid & 7) * 8;
    const bool pc_ok = p0 + lc < P, qc_ok = q0 + lc < Q;
    uint4 rl[2], rr[2];
    auto fetch = [&](int64_t ts) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t t = ts + lr + h * 32;
            const bool t_ok = t < tend;
            rl[h] = (t_ok && pc_ok) ? *reinterpret_cast<const uint4*>(L + t * ldl + p0 + lc) : make_uint4(0, 0, 0, 0);
            rr[h] = (t_ok && qc_ok) ? *reinterpret_cast<const uint4*>(R + t * ldr + q0 + lc) : make_uint4(0, 0, 0, 0);
        }
    };
    f32x4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (tbeg < tend) fetch(tbeg);
    for (int64_t ts = tbeg; ts < tend; ts += 64) {
        __syncthreads();                                      // the previous stage's fragments have been read
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            *reinterpret_cast<uint4*>(&sL[(lr + h * 32) * LORA_WG_LD + lc]) = rl[h];
            *reinterpret_cast<uint4*>(&sR[(lr + h * 32) * LORA_WG_LD + lc]) = rr[h];
        }
        __syncthreads();
        if (ts + 64 < tend) fetch(ts + 64);
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int idx = wave + 4 * s;
            if (idx < PT * QT) {
                const int pi = idx / QT, qi = idx % QT;
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    short8 a, b;
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const int tl = ks * 32 + g * 8 + i;
                        a[i] = (short)sL[tl * LORA_WG_LD + pi * 16 + m];
                        b[i] = (short)sR[tl * LORA_WG_LD + qi * 16 + m];
                    }
                    acc[s] = Mma<T>::mma(a, b, acc[s]);
                }
            }
        }
    }
    float* slab = ws + (int64_t)blockIdx.y * P * Q;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const int idx = wave + 4 * s;
        if (idx < PT * QT) {
            const int pi = idx / QT, qi = idx % QT;
            const int q = q0 + qi * 16 + m;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int p = p0 + pi * 16 + g * 4 + i;
                if (p < P && q < Q) slab[(int64_t)p * Q + q] = acc[s][i];
            }
        }
    }
}

// out[p, q] = alpha * (((slab 0 + slab 1) + slab 2) + ...): the one and only order, whatever the grid did
__global__ __launch_bounds__(256) void lora_wgrad_reduce_k(const float* __restrict__ ws, float* __restrict__ out, int64_t ldo, int P, int Q, int splits, float alpha) {
    const int64_t n = (int64_t)P * Q;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float v = ws[e];
    for (int s = 1; s < splits; ++s) v += ws[(int64_t)s * n + e];
    out[(e / Q) * ldo + (e % Q)] = alpha * v;
}

#define LORA_UNSUPPORTED(cond, ...) do { if (!(cond)) { ctmi_set_error(__VA_ARGS__); return CTMI_ERR_UNSUPPORTED; } } while (0)

void wgrad_plan(int64_t T, int64_t P, int64_t Q, int* splits, int* chunk) {
    const int64_t tiles = cdiv64(P, 64) * cdiv64(Q, 64);
    const int64_t stages = cdiv64(T, 64);
    int64_t want = cdiv64(1024, tiles);                     // about four workgroups per CU
    if (want > 32) want = 32;
    if (want > stages) want = stages;
    if (want < 1) want = 1;
    *chunk = (int)cdiv64(stages, want);
    *splits = (int)cdiv64(stages, *chunk);
}

template <typename T, bool KM>
void launch_project(const void* x, int64_t ldx, const void* w, int64_t ldw, void* out, int64_t ldo, int64_t Trows, int K, int r, float alpha, hipStream_t st) {
    const dim3 grid((unsigned)cdiv64(Trows, 16)), block(256);
    const T* X = (const T*)x; const T* W = (const T*)w; T* O = (T*)out;
    switch ((r + 15) / 16) {
        case 1: hipLaunchKernelGGL((lora_project_k<T, 1, KM>), grid, block, 0, st, X, ldx, W, ldw, O, ldo, Trows, K, r, alpha); break;
        case 2: hipLaunchKernelGGL((lora_project_k<T, 2, KM>), grid, block, 0, st, X, ldx, W, ldw, O, ldo, Trows, K, r, alpha); break;
        case 3: hipLaunchKernelGGL((lora_project_k<T, 3, KM>), grid, block, 0, st, X, ldx, W, ldw, O, ldo, Trows, K, r, alpha); break;
        default: hipLaunchKernelGGL((lora_project_k<T, 4, KM>), grid, block, 0, st, X, ldx, W, ldw, O, ldo, Trows, K, r, alpha); break;
    }
}

template <typename T, bool KM>
void launch_expand(const void* xa, int64_t ldxa, const void* w, int64_t ldw, void* y, int64_t ldy, int64_t Trows, int N, int r, hipStream_t st) {
    const dim3 grid((unsigned)cdiv64(N, 256), (unsigned)cdiv64(Trows, LORA_EXP_ROWS)), block(256);
    const T* X = (const T*)xa; const T* W = (const T*)w; T* Y = (T*)y;
    if (r <= 32) hipLaunchKernelGGL((lora_expand_add_k<T, 1, KM>), grid, block, 0, st, X, ldxa, W, ldw, Y, ldy, Trows, N, r);
    else         hipLaunchKernelGGL((lora_expand_add_k<T, 2, KM>), grid, block, 0, st, X, ldxa, W, ldw, Y, ldy, Trows, N, r);
}

// the (bf16 | fp16) x (W row-major | k-major) choice of project and expand-add: f(T{}, bool constant KMAJOR)
template <typename F> int by_dtype_layout(int dtype, int w_kmajor, const char* who, F&& f) {
    return ctmi_by_dtype16(dtype, who, [&](auto t) -> int { return w_kmajor ? f(t, std::true_type{}) : f(t, std::false_type{}); });
}

}  // namespace

extern "C" int ctmi_lora_project(const void* x, int64_t ldx, const void* w, int64_t ldw, int w_kmajor, void* out, int64_t ldo,
                                 int64_t T, int64_t K, int64_t r, float alpha, int dtype, void* stream) {
    LORA_UNSUPPORTED(dtype == CTMI_BF16 || dtype == CTMI_F16, "lora_project: dtype %d (bf16 / fp16 only; fp32 goes through ctmi_gemm)", dtype);
    LORA_UNSUPPORTED(r >= 8 && r <= 64 && r % 8 == 0, "lora_project: r = %lld (a multiple of 8 in [8, 64])", (long long)r);
    LORA_UNSUPPORTED(T >= 1 && T < (1ll << 31) * 16 && K >= 8 && K % 8 == 0 && K < (1ll << 30), "lora_project: T = %lld, K = %lld (T >= 1, K a multiple of 8)", (long long)T, (long long)K);
    LORA_UNSUPPORTED(ldx >= K && ldx % 8 == 0 && ldo >= r && ldw >= (w_kmajor ? r : K) && ldw % 8 == 0,
                     "lora_project: leading dimensions %lld / %lld / %lld (multiples of 8, at least the row length)", (long long)ldx, (long long)ldw, (long long)ldo);
    LORA_UNSUPPORTED(x && w && out && aligned16(x) && aligned16(w), "lora_project: NULL or unaligned pointer (16 bytes)");
    hipStream_t st = as_stream(stream);
    return by_dtype_layout(dtype, w_kmajor, "lora_project", [&](auto t, auto km) -> int {
        launch_project<decltype(t), decltype(km)::value>(x, ldx, w, ldw, out, ldo, T, (int)K, (int)r, alpha, st);
        CTMI_CHECK_LAUNCH("lora_project");
        return CTMI_OK;
    });
}

extern "C" int ctmi_lora_expand_add(const void* xa, int64_t ldxa, const void* w, int64_t ldw, int w_kmajor, void* y, int64_t ldy,
                                    int64_t T, int64_t N, int64_t r, int dtype, void* stream) {
    LORA_UNSUPPORTED(dtype == CTMI_BF16 || dtype == CTMI_F16, "lora_expand_add: dtype %d (bf16 / fp16 only; fp32 goes through ctmi_gemm)", dtype);
    LORA_UNSUPPORTED(r >= 8 && r <= 64 && r % 8 == 0, "lora_expand_add: r = %lld (a multiple of 8 in [8, 64])", (long long)r);
    LORA_UNSUPPORTED(T >= 1 && cdiv64(T, LORA_EXP_ROWS) <= 65535 && N >= 8 && N % 8 == 0 && N < (1ll << 30), "lora_expand_add: T = %lld, N = %lld (T >= 1, N a multiple of 8)", (long long)T, (long long)N);
    LORA_UNSUPPORTED(ldxa >= r && ldxa % 8 == 0 && ldy >= N && ldy % 8 == 0 && ldw >= (w_kmajor ? N : r) && ldw % 8 == 0,
                     "lora_expand_add: leading dimensions %lld / %lld / %lld (multiples of 8, at least the row length)", (long long)ldxa, (long long)ldw, (long long)ldy);
    LORA_UNSUPPORTED(xa && w && y && aligned16(xa) && aligned16(w) && aligned16(y), "lora_expand_add: NULL or unaligned pointer (16 bytes)");
    hipStream_t st = as_stream(stream);
    return by_dtype_layout(dtype, w_kmajor, "lora_expand_add", [&](auto t, auto km) -> int {
        launch_expand<decltype(t), decltype(km)::value>(xa, ldxa, w, ldw, y, ldy, T, (int)N, (int)r, st);
        CTMI_CHECK_LAUNCH("lora_expand_add");
        return CTMI_OK;
    });
}

extern "C" int64_t ctmi_lora_wgrad_ws(int64_t T, int64_t P, int64_t Q) {
    if (T < 1 || P < 1 || Q < 1) return 0;
    int splits, chunk;
    wgrad_plan(T, P, Q, &splits, &chunk);
    return (int64_t)splits * P * Q;
}

extern "C" int ctmi_lora_wgrad(const void* l, int64_t ldl, const void* r, int64_t ldr, float* out, int64_t ldo, int64_t T, int64_t P, int64_t Q,
                               float alpha, float* ws, int64_t ws_bytes, int dtype, void* stream) {
    LORA_UNSUPPORTED(dtype == CTMI_BF16 || dtype == CTMI_F16, "lora_wgrad: dtype %d (bf16 / fp16 only; fp32 goes through ctmi_gemm)", dtype);
    LORA_UNSUPPORTED(P >= 8 && Q >= 8 && P % 8 == 0 && Q % 8 == 0 && (P <= 64 || Q <= 64) && P < (1ll << 24) && Q < (1ll << 24),
                     "lora_wgrad: P = %lld, Q = %lld (multiples of 8, the smaller at most 64)", (long long)P, (long long)Q);
    LORA_UNSUPPORTED(T >= 1 && T < (1ll << 40), "lora_wgrad: T = %lld", (long long)T);
    LORA_UNSUPPORTED(ldl >= P && ldl % 8 == 0 && ldr >= Q && ldr % 8 == 0 && ldo >= Q, "lora_wgrad: leading dimensions %lld / %lld / %lld", (long long)ldl, (long long)ldr, (long long)ldo);
    LORA_UNSUPPORTED(l && r && out && ws && aligned16(l) && aligned16(r), "lora_wgrad: NULL or unaligned pointer (16 bytes)");
    int splits, chunk;
    wgrad_plan(T, P, Q, &splits, &chunk);
    LORA_UNSUPPORTED(ws_bytes >= (int64_t)splits * P * Q * 4, "lora_wgrad: workspace of %lld bytes, needs %lld (ctmi_lora_wgrad_ws floats)", (long long)ws_bytes,
                     (long long)splits * P * Q * 4);
    hipStream_t st = as_stream(stream);
    const int qtiles = (int)cdiv64(Q, 64);
    const dim3 grid((unsigned)(cdiv64(P, 64) * qtiles), (unsigned)splits), block(256);
    const int rc = ctmi_by_dtype16(dtype, "lora_wgrad", [&](auto t) -> int {
        using TT = decltype(t);
        hipLaunchKernelGGL((lora_wgrad_k<TT>), grid, block, 0, st, (const TT*)l, ldl, (const TT*)r, ldr, ws, T, (int)P, (int)Q, qtiles, chunk);
        CTMI_CHECK_LAUNCH("lora_wgrad");
        return CTMI_OK;
    });
    if (rc != CTMI_OK) return rc;
    hipLaunchKernelGGL(lora_wgrad_reduce_k, dim3((unsigned)cdiv64(P * Q, 256)), block, 0, st, ws, out, ldo, (int)P, (int)Q, splits, alpha);
    CTMI_CHECK_LAUNCH("lora_wgrad_reduce");
    return CTMI_OK;
}
