// LayerNorm forward / backward, the column sums of the bias gradients, and the multi-job reduction of their partial rows.
// gfx950: one wave (64 lanes) per row, the row in registers, 16-byte loads, fp32 statistics, wavefront shuffles for the reductions.
#include "common.h"
#include "reduce_jobs.h"
#include "prof.h"

// ------------------------------------------------------------------------------------------------
// LayerNorm  (transformer.py:71-89)
// ------------------------------------------------------------------------------------------------
// Fast path: one wave per row, the row cached in registers (MAXV 16-byte vectors per lane).
template <typename T, int MAXV>
__global__ __launch_bounds__(256) void ln_fwd_vec(const T* __restrict__ x, const float* __restrict__ w,
                                                  const float* __restrict__ b, T* __restrict__ y,
                                                  float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                  int64_t rows, int cols, float eps) {
    constexpr int VEC = 16 / sizeof(T);
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const float inv_n = 1.0f / (float)cols;
    for (int64_t row = wave0; row < rows; row += nwaves) {
        const T* xr = x + row * cols;
        float vals[MAXV][VEC];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VEC;
            if (c < cols) {
                uint4 r = *reinterpret_cast<const uint4*>(xr + c);
                unpack16<T>(r, vals[i]);
#pragma unroll
                for (int j = 0; j < VEC; ++j) s += vals[i][j];
            }
        }
        const float mean = wave_sum(s) * inv_n;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VEC;
            if (c < cols) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) { float d = vals[i][j] - mean; q += d * d; }
            }
        }
        const float var = wave_sum(q) * inv_n;
        const float rstd = 1.0f / sqrtf(var + eps);
        if (lane == 0) { mean_o[row] = mean; rstd_o[row] = rstd; }
        T* yr = y + row * cols;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VEC;
            if (c < cols) {
                float o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) o[j] = w[c + j] * ((vals[i][j] - mean) * rstd) + b[c + j];
                st_wt16(yr + c, pack16<T>(o));                           // (write-through: common.h)
            }
        }
    }
}

// Generic path (any cols / alignment): scalar loads, the row is re-read (L1/L2 hits).
template <typename T>
__global__ __launch_bounds__(256) void ln_fwd_gen(const T* __restrict__ x, const float* __restrict__ w,
                                                  const float* __restrict__ b, T* __restrict__ y,
                                                  float* __restrict__ mean_o, float* __restrict__ rstd_o,
                                                  int64_t rows, int64_t cols, float eps) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const float inv_n = 1.0f / (float)cols;
    for (int64_t row = wave0; row < rows; row += nwaves) {
        const T* xr = x + row * cols;
        float s = 0.f;
        for (int64_t c = lane; c < cols; c += 64) s += Cvt<T>::to_f(xr[c]);
        const float mean = wave_sum(s) * inv_n;
        float q = 0.f;
        for (int64_t c = lane; c < cols; c += 64) { float d = Cvt<T>::to_f(xr[c]) - mean; q += d * d; }
        const float rstd = 1.0f / sqrtf(wave_sum(q) * inv_n + eps);
        if (lane == 0) { mean_o[row] = mean; rstd_o[row] = rstd; }
        T* yr = y + row * cols;
        for (int64_t c = lane; c < cols; c += 64)
            yr[c] = Cvt<T>::from_f(w[c] * ((Cvt<T>::to_f(xr[c]) - mean) * rstd) + b[c]);
    }
}

template <typename T>
static int ln_fwd_launch(const void* x, const float* w, const float* b, void* y, float* mean, float* rstd,
                         int64_t rows, int64_t cols, float eps, hipStream_t st) {
    constexpr int VEC = 16 / sizeof(T);
    const bool vec_ok = (cols % VEC == 0) && aligned16(x) && aligned16(y);
    int grid = (int)std::min<int64_t>(cdiv64(rows, 4), 2048);
    if (grid < 1) grid = 1;
    const T* xp = (const T*)x; T* yp = (T*)y;
#define LN_FWD_CASE(MV) if (vec_ok && cols <= (int64_t)MV * 64 * VEC) { \
        hipLaunchKernelGGL((ln_fwd_vec<T, MV>), dim3(grid), dim3(256), 0, st, xp, w, b, yp, mean, rstd, rows, (int)cols, eps); \
        CTMI_CHECK_LAUNCH("layernorm_fwd"); return CTMI_OK; }
    LN_FWD_CASE(1) LN_FWD_CASE(2) LN_FWD_CASE(4) LN_FWD_CASE(8)
#undef LN_FWD_CASE
    hipLaunchKernelGGL((ln_fwd_gen<T>), dim3(grid), dim3(256), 0, st, xp, w, b, yp, mean, rstd, rows, cols, eps);
    CTMI_CHECK_LAUNCH("layernorm_fwd");
    return CTMI_OK;
}

extern "C" int ctmi_layernorm_fwd(const void* x, const float* w, const float* b, void* y, float* mean, float* rstd,
                                  int64_t rows, int64_t cols, float eps, int dtype, void* stream) {
    ProfScope prof__(CTMI_PROF_LAYERNORM, as_stream(stream));
    CTMI_REQUIRE(x && w && b && y && mean && rstd, "layernorm_fwd: null pointer");
    CTMI_REQUIRE(rows >= 0 && cols > 0, "layernorm_fwd: bad shape rows=%lld cols=%lld", (long long)rows, (long long)cols);
    if (rows == 0) return CTMI_OK;
    return ctmi_by_dtype(dtype, "layernorm_fwd", [&](auto t) {
        return ln_fwd_launch<decltype(t)>(x, w, b, y, mean, rstd, rows, cols, eps, as_stream(stream));
    });
}

// Backward.  dx = rstd * (g - mean(g) - xhat*mean(g*xhat)),  g = dy*w, xhat = (x-mean)*rstd.
// Each wave keeps per-lane partial sums of dw = sum dy*xhat and db = sum dy for its rows; a block combines its
// 4 waves through LDS and writes one partial row to ws[blockIdx][2][cols]; ln_bwd_reduce sums the partial rows.
// waves per workgroup in ln_bwd_vec: 8 for rows up to 64*VEC*2 elements, fewer for wider rows so the per-wave dw/db partials
// ([waves][2][cols] fp32 in LDS) stay within 64 KiB
static constexpr int lnb_waves(int maxv) { return maxv <= 2 ? 8 : (16 / maxv); }
// NS = 2: partial rows {dw, db};  NS = 4: additionally {colsum(dres), colsum(dx)} — the bias gradients of the two Linear layers
// whose output gradients this kernel already reads (dres) and writes (dx), so no separate column-sum pass over them exists.
// FULL: cols == MAXV * 64 * VEC exactly (no column guards) and RESM = 0 / 1: `dres` known absent / present at compile time — a loop body without
// control flow, in which hipcc counts its vector-memory operations exactly: with the guards its wait at the loop head was `vmcnt(0)`, i.e. the
// acknowledgement of the previous row's STORES was waited for before the next loads were issued.  RESM = -1: decided at run time (any width).
template <typename T, int MAXV, int NS = 2, bool FULL = false, int RESM = -1>
__global__ __launch_bounds__(64 * lnb_waves(MAXV)) void ln_bwd_vec(const T* __restrict__ dy, const T* __restrict__ x,
                                                  const float* __restrict__ w, const float* __restrict__ mean_i,
                                                  const float* __restrict__ rstd_i, const T* __restrict__ dres,
                                                  T* __restrict__ dx, float* __restrict__ ws, int64_t rows, int cols) {
    constexpr int VEC = 16 / sizeof(T);
    const bool has_res = RESM < 0 ? dres != nullptr : RESM == 1;
    constexpr int LNB_WAVES = lnb_waves(MAXV);
    constexpr int NX = NS == 4 ? MAXV : 1;                             // extra accumulators exist only for NS = 4
    float ar[NX][VEC], ax[NX][VEC];
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
        for (int j = 0; j < VEC; ++j) { ar[i][j] = 0.f; ax[i][j] = 0.f; }
    extern __shared__ __attribute__((aligned(16))) float lds[];      // [LNB_WAVES][2][cols]
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t wave0 = (int64_t)blockIdx.x * LNB_WAVES + wid;
    const int64_t nwaves = (int64_t)gridDim.x * LNB_WAVES;
    const float inv_n = 1.0f / (float)cols;
    float aw[MAXV][VEC], ab[MAXV][VEC], wv[MAXV][VEC];
#pragma unroll
    for (int i = 0; i < MAXV; ++i) {
        const int c = (i * 64 + lane) * VEC;
#pragma unroll
        for (int j = 0; j < VEC; ++j) { aw[i][j] = 0.f; ab[i][j] = 0.f; wv[i][j] = (FULL || c < cols) ? w[c + j] : 0.f; }
    }
    // all three input rows are requested before anything is reduced (the residual-gradient row is only needed after the two wave
    // reductions, and loaded there it exposed a full HBM latency per row) — and, round 4, one row AHEAD: the loads of the wave's next row
    // are in flight while this row is reduced and stored (with 8 waves per CU a wave that waits for its own row leaves the memory pipe
    // idle half the time: 21.7 us for 64 MiB = 2.9 TB/s).  The row after the last is clamped to the last (loaded twice, used once).
    auto load_row = [&](int64_t r, uint4 (&xq)[MAXV], uint4 (&gq)[MAXV], uint4 (&rq)[MAXV], float& mu, float& rs) {
        mu = mean_i[r]; rs = rstd_i[r];
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VEC;
            if (FULL || c < cols) {
                xq[i] = *reinterpret_cast<const uint4*>(x + r * cols + c);
                gq[i] = *reinterpret_cast<const uint4*>(dy + r * cols + c);
                if (has_res) rq[i] = *reinterpret_cast<const uint4*>(dres + r * cols + c);
            }
        }
    };
    // one row: the two wave reductions, dx (+ residual gradient), the per-lane partial sums.  `valid` = false (the clamped row after the last,
    // second half of a two-row trip): nothing is stored and dy counts as zero, so the partial sums do not move.
    auto process = [&](const uint4 (&xraw)[MAXV], const uint4 (&graw)[MAXV], const uint4 (&rraw)[MAXV], float mean, float rstd, int64_t row, bool valid) {
        float xh[MAXV][VEC], g[MAXV][VEC];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VEC;
            if (FULL || c < cols) {
                float xv[VEC], dv[VEC];
                unpack16<T>(xraw[i], xv);
                unpack16<T>(graw[i], dv);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    if (!valid) dv[j] = 0.f;
                    xh[i][j] = (xv[j] - mean) * rstd;
                    g[i][j] = dv[j] * wv[i][j];
                    s1 += g[i][j];
                    s2 += g[i][j] * xh[i][j];
                    aw[i][j] += dv[j] * xh[i][j];
                    ab[i][j] += dv[j];
                }
            }
        }
        s1 = wave_sum(s1) * inv_n;
        s2 = wave_sum(s2) * inv_n;
        T* dxr = dx + row * cols;
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VEC;
            if (FULL || c < cols) {
                float o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) o[j] = rstd * (g[i][j] - s1 - xh[i][j] * s2);
                if (has_res) {
                    float r[VEC];
                    unpack16<T>(rraw[i], r);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) { if (!valid) r[j] = 0.f; o[j] += r[j]; if (NS == 4) ar[NS == 4 ? i : 0][j] += r[j]; }
                }
                const uint4 pk = pack16<T>(o);
                if (valid) st_wt16(dxr + c, pk);
                if (NS == 4) {                                           // column sums of dx as STORED (what the weight-gradient GEMM reads)
                    float orr[VEC];
                    unpack16<T>(pk, orr);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) ax[NS == 4 ? i : 0][j] += valid ? orr[j] : 0.f;
                }
            }
        }
    };
    // the loads of the next row stay in flight while the current one is reduced and stored (round 4)
    // (NS = 4 keeps one row at a time: with 32 more accumulators the two-set form needs all 256 registers and spills)
    if (NS == 2) {
        // two rows per trip over two register sets (A, B) — no copies between them: a copy of the prefetched row into "current" registers is
        // where hipcc placed its wait, i.e. at the bottom of the trip that had just issued the loads
        uint4 xa[MAXV], ga[MAXV], ra[MAXV], xb[MAXV], gb[MAXV], rb[MAXV];
        float mean_a = 0.f, rstd_a = 0.f, mean_b = 0.f, rstd_b = 0.f;
        if (wave0 < rows) load_row(wave0, xa, ga, ra, mean_a, rstd_a);
        for (int64_t row = wave0; row < rows; row += 2 * nwaves) {
            const int64_t r1 = row + nwaves, r1c = min(r1, rows - 1);
            load_row(r1c, xb, gb, rb, mean_b, rstd_b);
            process(xa, ga, ra, mean_a, rstd_a, row, true);
            load_row(min(row + 2 * nwaves, rows - 1), xa, ga, ra, mean_a, rstd_a);
            process(xb, gb, rb, mean_b, rstd_b, r1c, r1 < rows);
        }
    } else {
        for (int64_t row = wave0; row < rows; row += nwaves) {
            uint4 xraw[MAXV], graw[MAXV], rraw[MAXV];
            float mean, rstd;
            load_row(row, xraw, graw, rraw, mean, rstd);
            process(xraw, graw, rraw, mean, rstd, row, true);
        }
    }
    // block combine, two partial rows per pass through the [LNB_WAVES][2][cols] LDS patch
    float* out = ws + (int64_t)blockIdx.x * NS * cols;
#pragma unroll
    for (int pass = 0; pass < NS / 2; ++pass) {
        if (pass) __syncthreads();
#pragma unroll
        for (int i = 0; i < MAXV; ++i) {
            const int c = (i * 64 + lane) * VEC;
            if (FULL || c < cols) {
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    lds[(wid * 2 + 0) * cols + c + j] = pass == 0 ? aw[i][j] : ar[NS == 4 ? i : 0][j];
                    lds[(wid * 2 + 1) * cols + c + j] = pass == 0 ? ab[i][j] : ax[NS == 4 ? i : 0][j];
                }
            }
        }
        __syncthreads();
        for (int c = threadIdx.x; c < 2 * cols; c += 64 * LNB_WAVES) {
            const int which = c / cols, cc = c - which * cols;
            float t = 0.f;
#pragma unroll
            for (int k = 0; k < LNB_WAVES; ++k) t += lds[(k * 2 + which) * cols + cc];
            out[pass * 2 * cols + c] = t;
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void ln_bwd_gen(const T* __restrict__ dy, const T* __restrict__ x,
                                                  const float* __restrict__ w, const float* __restrict__ mean_i,
                                                  const float* __restrict__ rstd_i, const T* __restrict__ dres,
                                                  T* __restrict__ dx, int64_t rows, int64_t cols) {
    const int lane = threadIdx.x & 63;
    const int64_t wave0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t nwaves = (int64_t)gridDim.x * 4;
    const float inv_n = 1.0f / (float)cols;
    for (int64_t row = wave0; row < rows; row += nwaves) {
        const float mean = mean_i[row], rstd = rstd_i[row];
        const T* xr = x + row * cols;
        const T* gr = dy + row * cols;
        float s1 = 0.f, s2 = 0.f;
        for (int64_t c = lane; c < cols; c += 64) {
            float g = Cvt<T>::to_f(gr[c]) * w[c];
            s1 += g; s2 += g * ((Cvt<T>::to_f(xr[c]) - mean) * rstd);
        }
        s1 = wave_sum(s1) * inv_n; s2 = wave_sum(s2) * inv_n;
        for (int64_t c = lane; c < cols; c += 64) {
            float xh = (Cvt<T>::to_f(xr[c]) - mean) * rstd;
            float o = rstd * (Cvt<T>::to_f(gr[c]) * w[c] - s1 - xh * s2);
            if (dres != nullptr) o += Cvt<T>::to_f(dres[row * cols + c]);
            dx[row * cols + c] = Cvt<T>::from_f(o);
        }
    }
}

// generic dw/db partials: block b handles rows [b*chunk, (b+1)*chunk); thread per column.
template <typename T>
__global__ __launch_bounds__(256) void ln_bwd_wb_gen(const T* __restrict__ dy, const T* __restrict__ x,
                                                     const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                     float* __restrict__ ws, int64_t rows, int64_t cols, int64_t chunk) {
    const int64_t r0 = (int64_t)blockIdx.x * chunk, r1 = min(rows, r0 + chunk);
    float* out = ws + (int64_t)blockIdx.x * 2 * cols;
    for (int64_t c = threadIdx.x; c < cols; c += 256) {
        float aw = 0.f, ab = 0.f;
        for (int64_t r = r0; r < r1; ++r) {
            float d = Cvt<T>::to_f(dy[r * cols + c]);
            aw += d * ((Cvt<T>::to_f(x[r * cols + c]) - mean_i[r]) * rstd_i[r]);
            ab += d;
        }
        out[c] = aw; out[cols + c] = ab;
    }
}

// Wide rows (more than 4 x 64 16-byte chunks: hidden sizes above 2048 in bf16): one 4-wave workgroup per row, each wave
// owning every 4th 1-KiB chunk, so a lane keeps MVW chunks of x / dy / the dw,db partials in registers instead of 8 (the
// one-wave-per-row kernel needs all 256 VGPRs there and leaves one wave per SIMD).  The two row sums cross the waves through
// LDS (double-buffered by row parity: one barrier per row).  Partials: ws[block][2][cols], no cross-wave combine.
template <typename T, int MVW>
__global__ __launch_bounds__(256) void ln_bwd_wide(const T* __restrict__ dy, const T* __restrict__ x, const float* __restrict__ w,
                                                   const float* __restrict__ mean_i, const float* __restrict__ rstd_i,
                                                   const T* __restrict__ dres, T* __restrict__ dx, float* __restrict__ ws,
                                                   int64_t rows, int cols) {
    constexpr int VEC = 16 / sizeof(T);
    __shared__ float sm[2][2][4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const float inv_n = 1.0f / (float)cols;
    float aw[MVW][VEC], ab[MVW][VEC], wvv[MVW][VEC];
    int col[MVW];
#pragma unroll
    for (int i = 0; i < MVW; ++i) {
        col[i] = ((i * 4 + wv) * 64 + lane) * VEC;
#pragma unroll
        for (int j = 0; j < VEC; ++j) { aw[i][j] = 0.f; ab[i][j] = 0.f; wvv[i][j] = (col[i] < cols) ? w[col[i] + j] : 0.f; }
    }
    int par = 0;
    for (int64_t row = blockIdx.x; row < rows; row += gridDim.x, par ^= 1) {
        const float mean = mean_i[row], rstd = rstd_i[row];
        uint4 xraw[MVW], graw[MVW], rraw[MVW];
#pragma unroll
        for (int i = 0; i < MVW; ++i)
            if (col[i] < cols) {
                xraw[i] = *reinterpret_cast<const uint4*>(x + row * cols + col[i]);
                graw[i] = *reinterpret_cast<const uint4*>(dy + row * cols + col[i]);
                if (dres != nullptr) rraw[i] = *reinterpret_cast<const uint4*>(dres + row * cols + col[i]);
            }
        float xh[MVW][VEC], g[MVW][VEC];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < MVW; ++i) {
            if (col[i] < cols) {
                float xv[VEC], dv[VEC];
                unpack16<T>(xraw[i], xv);
                unpack16<T>(graw[i], dv);
#pragma unroll
                for (int j = 0; j < VEC; ++j) {
                    xh[i][j] = (xv[j] - mean) * rstd;
                    g[i][j] = dv[j] * wvv[i][j];
                    s1 += g[i][j];
                    s2 += g[i][j] * xh[i][j];
                    aw[i][j] += dv[j] * xh[i][j];
                    ab[i][j] += dv[j];
                }
            }
        }
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        if (lane == 0) { sm[par][0][wv] = s1; sm[par][1][wv] = s2; }
        __syncthreads();
        s1 = (sm[par][0][0] + sm[par][0][1] + sm[par][0][2] + sm[par][0][3]) * inv_n;
        s2 = (sm[par][1][0] + sm[par][1][1] + sm[par][1][2] + sm[par][1][3]) * inv_n;
#pragma unroll
        for (int i = 0; i < MVW; ++i) {
            if (col[i] < cols) {
                float o[VEC];
#pragma unroll
                for (int j = 0; j < VEC; ++j) o[j] = rstd * (g[i][j] - s1 - xh[i][j] * s2);
                if (dres != nullptr) {
                    float r[VEC];
                    unpack16<T>(rraw[i], r);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) o[j] += r[j];
                }
                *reinterpret_cast<uint4*>(dx + row * cols + col[i]) = pack16<T>(o);
            }
        }
    }
    float* out = ws + (int64_t)blockIdx.x * 2 * cols;
#pragma unroll
    for (int i = 0; i < MVW; ++i)
        if (col[i] < cols) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) { out[col[i] + j] = aw[i][j]; out[cols + col[i] + j] = ab[i][j]; }
        }
}

__global__ __launch_bounds__(256) void ln_bwd_reduce(const float* __restrict__ ws, float* __restrict__ dw,
                                                     float* __restrict__ db, int nparts, int64_t cols, int accumulate) {
    // 64 columns x 4 row-slices per block; blockIdx.y selects dw / db
    __shared__ float sm[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * 64 + tx;
    const int which = blockIdx.y;
    float t = 0.f;
    if (c < cols) {
#pragma unroll 8
        for (int p = ty; p < nparts; p += 4) t += ws[((int64_t)p * 2 + which) * cols + c];
    }
    sm[ty][tx] = t;
    __syncthreads();
    if (ty == 0 && c < cols) {
        float r = sm[0][tx] + sm[1][tx] + sm[2][tx] + sm[3][tx];
        float* o = which ? db : dw;
        o[c] = accumulate ? o[c] + r : r;
    }
}
// the same for wide rows (cols % 256 == 0): a lane sums 4 adjacent columns with 16-byte loads, so a wave reads 1 KiB of each
// partial row instead of 256 B (the partial rows are 2*cols*4 bytes apart: 256-byte pieces of them ran at ~40 GB/s)
__global__ __launch_bounds__(256) void ln_bwd_reduce4(const float* __restrict__ ws, float* __restrict__ dw,
                                                      float* __restrict__ db, int nparts, int64_t cols, int accumulate) {
    __shared__ float4 sm[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t c = ((int64_t)blockIdx.x * 64 + tx) * 4;
    const int which = blockIdx.y;
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 8
    for (int p = ty; p < nparts; p += 4) {
        const float4 v = *reinterpret_cast<const float4*>(ws + ((int64_t)p * 2 + which) * cols + c);
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    sm[ty][tx] = t;
    __syncthreads();
    if (ty == 0) {
        float4 r = sm[0][tx];
#pragma unroll
        for (int k = 1; k < 4; ++k) { r.x += sm[k][tx].x; r.y += sm[k][tx].y; r.z += sm[k][tx].z; r.w += sm[k][tx].w; }
        float* o = (which ? db : dw) + c;
        if (accumulate) { r.x += o[0]; r.y += o[1]; r.z += o[2]; r.w += o[3]; }
        o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
    }
}

constexpr int LN_BWD_BLOCKS = 256;          // one workgroup per CU: same-box A/B vs 512: 31.0 -> 21.4 us at [8192,1024] bf16 (half the end-of-kernel LDS combines and partial rows)
static const int LN_BWD_MAX_BLOCKS = 512;                               // workspace sizing (fixed); the launch uses LN_BWD_BLOCKS <= this
extern "C" int64_t ctmi_layernorm_bwd_ws(int64_t rows, int64_t cols) {
    (void)rows;
    return (int64_t)LN_BWD_MAX_BLOCKS * 4 * cols;          // up to 4 partial rows per block (dw, db, colsum(dres), colsum(dx))
}

// Main pass only: dx (+ dres) and the per-block partial rows ws[part][NS][cols] (NS = 2: dw, db; NS = 4: + colsum(dres),
// colsum(dx) when `want_sums` and the row width has the vector kernel).  The caller reduces the partial rows
// (ln_bwd_reduce* below, or one ctmi_reduce_jobs launch for a whole transformer block).
template <typename T>
static int ln_bwd_parts(const void* dy, const void* x, const float* w, const float* mean, const float* rstd,
                        const void* dres, void* dx, float* ws, int64_t rows, int64_t cols, int want_sums,
                        int* nparts_out, int* ns_out, hipStream_t st) {
    constexpr int VEC = 16 / sizeof(T);
    const bool vec_ok = (cols % VEC == 0) && aligned16(x) && aligned16(dy) && aligned16(dx) &&
                        (dres == nullptr || aligned16(dres)) && cols <= 8LL * 64 * VEC;
    int nparts, ns = 2;
    if (vec_ok) {
        const int mv = cols <= 64 * VEC ? 1 : (cols <= 2 * 64 * VEC ? 2 : (cols <= 4 * 64 * VEC ? 4 : 8));
        const int nw = lnb_waves(mv);
        int grid = (int)std::min<int64_t>(cdiv64(rows, nw), LN_BWD_BLOCKS);
        if (mv >= 4) {                                                  // wide rows: one workgroup per row, columns split over 4 waves
            grid = (int)std::min<int64_t>(rows, LN_BWD_MAX_BLOCKS);
            if (mv == 4) hipLaunchKernelGGL((ln_bwd_wide<T, 1>), dim3(grid), dim3(256), 0, st, (const T*)dy, (const T*)x, w, mean, rstd, (const T*)dres, (T*)dx, ws, rows, (int)cols);
            else hipLaunchKernelGGL((ln_bwd_wide<T, 2>), dim3(grid), dim3(256), 0, st, (const T*)dy, (const T*)x, w, mean, rstd, (const T*)dres, (T*)dx, ws, rows, (int)cols);
        }
        nparts = grid;
        size_t lds = (size_t)cols * 2 * nw * sizeof(float);
#define LN_BWD_LAUNCH(MV, NSV, FL, RM) { \
            ctmi_dyn_lds(reinterpret_cast<const void*>(&ln_bwd_vec<T, MV, NSV, FL, RM>), lds); \
            hipLaunchKernelGGL((ln_bwd_vec<T, MV, NSV, FL, RM>), dim3(grid), dim3(64 * lnb_waves(MV)), lds, st, (const T*)dy, (const T*)x, w, mean, rstd, \
                               (const T*)dres, (T*)dx, ws, rows, (int)cols); }
#define LN_BWD_CASE(MV, NSV) { \
            if (cols == (int64_t)MV * 64 * VEC) { if (dres != nullptr) LN_BWD_LAUNCH(MV, NSV, true, 1) else LN_BWD_LAUNCH(MV, NSV, true, 0) } \
            else LN_BWD_LAUNCH(MV, NSV, false, -1) }
        if (mv >= 4) { (void)lds; }
        else if (want_sums) { ns = 4; if (mv == 1) LN_BWD_CASE(1, 4) else LN_BWD_CASE(2, 4) }
        else { if (mv == 1) LN_BWD_CASE(1, 2) else LN_BWD_CASE(2, 2) }
#undef LN_BWD_LAUNCH
#undef LN_BWD_CASE
        CTMI_CHECK_LAUNCH("layernorm_bwd");
    } else {
        int grid = (int)std::min<int64_t>(cdiv64(rows, 4), 2048);
        hipLaunchKernelGGL((ln_bwd_gen<T>), dim3(grid), dim3(256), 0, st, (const T*)dy, (const T*)x, w, mean, rstd,
                           (const T*)dres, (T*)dx, rows, cols);
        CTMI_CHECK_LAUNCH("layernorm_bwd");
        nparts = (int)std::min<int64_t>(rows, LN_BWD_MAX_BLOCKS);
        int64_t chunk = cdiv64(rows, nparts);
        nparts = (int)cdiv64(rows, chunk);
        hipLaunchKernelGGL((ln_bwd_wb_gen<T>), dim3(nparts), dim3(256), 0, st, (const T*)dy, (const T*)x, mean, rstd, ws, rows, cols, chunk);
        CTMI_CHECK_LAUNCH("layernorm_bwd_wb");
    }
    *nparts_out = nparts; *ns_out = ns;
    return CTMI_OK;
}

template <typename T>
static int ln_bwd_launch(const void* dy, const void* x, const float* w, const float* mean, const float* rstd,
                         const void* dres, void* dx, float* dw, float* db, int accumulate, float* ws,
                         int64_t rows, int64_t cols, hipStream_t st) {
    int nparts = 0, ns = 2;
    int rc = ln_bwd_parts<T>(dy, x, w, mean, rstd, dres, dx, ws, rows, cols, 0, &nparts, &ns, st);
    if (rc != CTMI_OK) return rc;
    if (cols % 256 == 0 && cols >= 2048 && aligned16(ws))
        hipLaunchKernelGGL(ln_bwd_reduce4, dim3((unsigned)(cols / 256), 2), dim3(256), 0, st, ws, dw, db, nparts, cols, accumulate);
    else
        hipLaunchKernelGGL(ln_bwd_reduce, dim3((unsigned)cdiv64(cols, 64), 2), dim3(256), 0, st, ws, dw, db, nparts, cols, accumulate);
    CTMI_CHECK_LAUNCH("layernorm_bwd_reduce");
    return CTMI_OK;
}

// internal (block.hip): main pass + partial rows only
int ctmi_ln_bwd_parts_internal(const void* dy, const void* x, const float* w, const float* mean, const float* rstd,
                               const void* dres, void* dx, float* ws, int64_t rows, int64_t cols, int dtype, int want_sums,
                               int* nparts, int* ns, hipStream_t st) {
    ProfScope prof__(CTMI_PROF_LAYERNORM, st);
    return ctmi_by_dtype(dtype, "layernorm_bwd", [&](auto t) {
        return ln_bwd_parts<decltype(t)>(dy, x, w, mean, rstd, dres, dx, ws, rows, cols, want_sums, nparts, ns, st);
    });
}

extern "C" int ctmi_layernorm_bwd(const void* dy, const void* x, const float* w, const float* mean, const float* rstd,
                                  const void* dres, void* dx, float* dw, float* db, int accumulate, float* ws,
                                  int64_t rows, int64_t cols, int dtype, void* stream) {
    ProfScope prof__(CTMI_PROF_LAYERNORM, as_stream(stream));
    CTMI_REQUIRE(dy && x && w && mean && rstd && dx && dw && db && ws, "layernorm_bwd: null pointer");
    CTMI_REQUIRE(rows > 0 && cols > 0, "layernorm_bwd: bad shape");
    return ctmi_by_dtype(dtype, "layernorm_bwd", [&](auto t) {
        return ln_bwd_launch<decltype(t)>(dy, x, w, mean, rstd, dres, dx, dw, db, accumulate, ws, rows, cols, as_stream(stream));
    });
}

// ------------------------------------------------------------------------------------------------
// column sum (bias gradients)
// ------------------------------------------------------------------------------------------------
static const int COLSUM_PARTS = 128;
extern "C" int64_t ctmi_colsum_ws(int64_t M, int64_t N) { (void)M; return (int64_t)COLSUM_PARTS * N; }

// grid (ceil(N/ (64*VEC)), parts): each block sums a slab of rows for 64*VEC columns, 4 waves over rows.
template <typename T>
__global__ __launch_bounds__(256) void colsum_part(const T* __restrict__ x, int64_t ld, float* __restrict__ ws,
                                                   int64_t M, int64_t N, int64_t rows_per_part, int vec_ok) {
    constexpr int VEC = 16 / sizeof(T);
    __shared__ float sm[4][64 * VEC];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t c0 = ((int64_t)blockIdx.x * 64 + lane) * VEC;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_part, r1 = min(M, r0 + rows_per_part);
    float acc[VEC];
#pragma unroll
    for (int j = 0; j < VEC; ++j) acc[j] = 0.f;
    if (vec_ok) {
        if (c0 < N) {
            int64_t r = r0 + wid;
            for (; r + 12 < r1; r += 16) {                                   // 4 independent 16-byte loads in flight per lane
                uint4 q[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) q[u] = *reinterpret_cast<const uint4*>(x + (r + 4 * u) * ld + c0);
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    float v[VEC];
                    unpack16<T>(q[u], v);
#pragma unroll
                    for (int j = 0; j < VEC; ++j) acc[j] += v[j];
                }
            }
            for (; r < r1; r += 4) {
                float v[VEC];
                unpack16<T>(*reinterpret_cast<const uint4*>(x + r * ld + c0), v);
#pragma unroll
                for (int j = 0; j < VEC; ++j) acc[j] += v[j];
            }
        }
    } else {
        for (int64_t r = r0 + wid; r < r1; r += 4)
#pragma unroll
            for (int j = 0; j < VEC; ++j) if (c0 + j < N) acc[j] += Cvt<T>::to_f(x[r * ld + c0 + j]);
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j) sm[wid][lane * VEC + j] = acc[j];
    __syncthreads();
    for (int i = threadIdx.x; i < 64 * VEC; i += 256) {
        const int64_t c = (int64_t)blockIdx.x * 64 * VEC + i;
        if (c < N) ws[(int64_t)blockIdx.y * N + c] = sm[0][i] + sm[1][i] + sm[2][i] + sm[3][i];
    }
}
// 64 columns x 4 part-slices per block, LDS combine (the parts loop is unrolled so its loads pipeline)
__global__ __launch_bounds__(256) void colsum_final(const float* __restrict__ ws, float* __restrict__ out, int parts,
                                                    int64_t N, int accumulate) {
    __shared__ float sm[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t c = (int64_t)blockIdx.x * 64 + tx;
    float t = 0.f;
    if (c < N) {
#pragma unroll 8
        for (int p = ty; p < parts; p += 4) t += ws[(int64_t)p * N + c];
    }
    sm[ty][tx] = t;
    __syncthreads();
    if (ty == 0 && c < N) {
        const float r = sm[0][tx] + sm[1][tx] + sm[2][tx] + sm[3][tx];
        out[c] = accumulate ? out[c] + r : r;
    }
}

// partial rows only: ws[part][N]; *parts_out partial rows
int ctmi_colsum_parts_internal(const void* x, int64_t ld, float* ws, int64_t M, int64_t N, int dtype, int* parts_out, hipStream_t st) {
    ProfScope prof__(CTMI_PROF_REDUCE, st);
    return ctmi_by_dtype(dtype, "colsum", [&](auto t) -> int {
        using T = decltype(t);
        constexpr int VEC = 16 / sizeof(T);
        const int64_t xblocks = cdiv64(N, 64 * VEC);
        // ~2048 workgroups (8 waves per SIMD) so the row streams cover the HBM latency; >= 16 rows per part
        int parts = (int)std::min<int64_t>(std::max<int64_t>(16, std::min<int64_t>(COLSUM_PARTS, cdiv64(2048, xblocks))), cdiv64(M, 16));
        const int64_t rpp = cdiv64(M, parts);
        parts = (int)cdiv64(M, rpp);
        const int vec_ok = (N % VEC == 0) && (ld % VEC == 0) && aligned16(x);
        hipLaunchKernelGGL((colsum_part<T>), dim3((unsigned)xblocks, parts), dim3(256), 0, st, (const T*)x, ld, ws, M, N, rpp, vec_ok);
        CTMI_CHECK_LAUNCH("colsum_part");
        *parts_out = parts;
        return CTMI_OK;
    });
}

extern "C" int ctmi_colsum(const void* x, int64_t ld, float* out, int accumulate, float* ws, int64_t M, int64_t N, int dtype, void* stream) {
    CTMI_REQUIRE(x && out && ws && M > 0 && N > 0, "colsum: bad args");
    hipStream_t st = as_stream(stream);
    int parts = 0;
    int rc = ctmi_colsum_parts_internal(x, ld, ws, M, N, dtype, &parts, st);
    if (rc != CTMI_OK) return rc;
    hipLaunchKernelGGL(colsum_final, dim3((unsigned)cdiv64(N, 64)), dim3(256), 0, st, ws, out, parts, N, accumulate);
    CTMI_CHECK_LAUNCH("colsum_final");
    return CTMI_OK;
}

// ------------------------------------------------------------------------------------------------
// multi-job partial-row reduction: dst[c] (+)= alpha * sum_p src[p * part_stride + c], c < n, for up to CTMI_REDUCE_MAX_JOBS
// independent jobs in ONE launch (fixed summation order: deterministic).  A transformer block's backward leaves the partial
// rows of its two LayerNorm backward passes and its bias column sums in workspaces and reduces them all here, instead of one
// small "final" launch per vector (what used to be 96 colsum_final + 50 ln_bwd_reduce launches per Bloom-560M step).
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reduce_jobs_k(ReduceJobs R) {
    __shared__ float sm[4][64];
    reduce_jobs_block(R, (int)blockIdx.x, sm);                            // (csrc/reduce_jobs.h: shared with gemm.hip's wgrad_tail_k)
}

extern "C" int ctmi_reduce_jobs(const ctmi_reduce_job* jobs, int count, void* stream) {
    ProfScope prof__(CTMI_PROF_REDUCE, as_stream(stream));
    CTMI_REQUIRE(jobs != nullptr && count >= 0, "reduce_jobs: bad args");
    hipStream_t st = as_stream(stream);
    for (int base = 0; base < count; base += CTMI_REDUCE_MAX_JOBS) {
        ReduceJobs R;
        const int chunks = reduce_jobs_pack(jobs + base, std::min(CTMI_REDUCE_MAX_JOBS, count - base), R);
        if (chunks < 0) return CTMI_ERR_ARG;
        hipLaunchKernelGGL(reduce_jobs_k, dim3((unsigned)chunks), dim3(256), 0, st, R);
        CTMI_CHECK_LAUNCH("reduce_jobs");
    }
    return CTMI_OK;
}
