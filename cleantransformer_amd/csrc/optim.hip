// Parameter-sized passes: fused multi-tensor AdamW / SGD, the GradScaler kernels, casts, transpose-cast, sum of squares, scale.
#include "common.h"
#include "prof.h"

// ------------------------------------------------------------------------------------------------
// fused multi-tensor AdamW / SGD   (optimizer.py:53-97, 12-50; torch.optim.AdamW semantics at ft_bloom.py:70)
// 28 B/param of HBM traffic (+2 B when the bf16 shadow is written, +4 B when the L2 form writes the grad back).
// ------------------------------------------------------------------------------------------------
struct MTPack {
    float* p[CTMI_MT_MAX];
    float* g[CTMI_MT_MAX];
    float* m[CTMI_MT_MAX];
    float* v[CTMI_MT_MAX];
    bf16_t* shadow[CTMI_MT_MAX];
    int64_t n[CTMI_MT_MAX];
};
struct AdamHyper { float lr, b1, b2, eps, wd, bc1, bc2, sqrt_bc2, gscale; int decoupled, mutate_grad, shadow_f16; };

__device__ __forceinline__ void adam_one(float& p, float& g, float& m, float& v, const AdamHyper& h) {
    // no FMA contraction: every launch form, and the vector and scalar paths of one launch, round every product and sum the same way — the
    // update of an element does not depend on which kernel (or which lane of it) happened to process it
#pragma clang fp contract(off)
    g *= h.gscale;
    if (h.decoupled) { p *= (1.0f - h.lr * h.wd); } else { g += h.wd * p; }
    m = h.b1 * m + (1.0f - h.b1) * g;
    v = h.b2 * v + (1.0f - h.b2) * g * g;
    if (h.decoupled) p -= (h.lr / h.bc1) * (m / (sqrtf(v) / h.sqrt_bc2 + h.eps));
    else             p -= h.lr * (m / h.bc1) / (sqrtf(v / h.bc2) + h.eps);
}

__global__ __launch_bounds__(256) void adamw_mt_k(MTPack pk, AdamHyper h) {
    const int ti = blockIdx.y;
    const int64_t n = pk.n[ti];
    float* __restrict__ p = pk.p[ti]; float* __restrict__ g = pk.g[ti];
    float* __restrict__ m = pk.m[ti]; float* __restrict__ v = pk.v[ti];
    bf16_t* __restrict__ sh = pk.shadow[ti];
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) && (sh == nullptr || (((uintptr_t)sh) & 7) == 0);
    const int64_t n4 = vec ? (n / 4) : 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 P = ldg_stream(p + 4 * i), G = ldg_stream(g + 4 * i);
        float4 M = ldg_stream(m + 4 * i), V = ldg_stream(v + 4 * i);
        adam_one(P.x, G.x, M.x, V.x, h); adam_one(P.y, G.y, M.y, V.y, h);
        adam_one(P.z, G.z, M.z, V.z, h); adam_one(P.w, G.w, M.w, V.w, h);
        stg_stream(p + 4 * i, P); stg_stream(m + 4 * i, M); stg_stream(v + 4 * i, V);
        if (h.mutate_grad) stg_stream(g + 4 * i, G);
        // the operand copy of the weights in the compute dtype (bf16, or IEEE half since round 5), written in the same pass
        if (sh) reinterpret_cast<uint2*>(sh)[i] = h.shadow_f16 ? make_uint2(pack_h2(P.x, P.y), pack_h2(P.z, P.w)) : make_uint2(pack_bf2(P.x, P.y), pack_bf2(P.z, P.w));
    }
    for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        float P = p[i], G = g[i], M = m[i], V = v[i];
        adam_one(P, G, M, V, h);
        p[i] = P; m[i] = M; v[i] = V;
        if (h.mutate_grad) g[i] = G;
        if (sh) sh[i] = h.shadow_f16 ? f2h(P).v : f2bf(P);
    }
}

// Chunk-balanced form (round 6): up to CTMI_MT_FLAT tensors per launch, a 1-D grid of one 16 Ki-element chunk per workgroup (64 KiB of every
// fp32 stream; 4 x 16-byte loads per stream and thread in flight).  The (x = stride loop, y = tensor) grid above gives every tensor of a pack
// the workgroups of the LARGEST one — a pack of the 257 M-element tied table and 23 small vectors launches 24 x 2048 workgroups of which 23 x
// ~2040 exit at once — and the 294 parameters of Bloom-560M took 13 launches; here it is 5, every workgroup with the same amount of work.
#define CTMI_MT_FLAT 64
constexpr int ADAM_CHUNK = 16384;                          // elements per workgroup: 256 threads x 4 float4 x 4
struct MTFlat {
    float* p[CTMI_MT_FLAT]; float* g[CTMI_MT_FLAT]; float* m[CTMI_MT_FLAT]; float* v[CTMI_MT_FLAT];
    bf16_t* shadow[CTMI_MT_FLAT];
    int64_t n[CTMI_MT_FLAT];
    int first[CTMI_MT_FLAT + 1];                           // first chunk of tensor i in this launch's grid
    int count;
};
// DEV: the hyper-parameters (with this step's bias corrections) are read from device memory — the form a captured hipGraph replays: the launch's
// arguments are frozen at capture, the record behind `hd` is rewritten before every replay (ctmi_adamw_set_hyper)
template <bool DEV>
__global__ __launch_bounds__(256) void adamw_flat_k(MTFlat pk, AdamHyper hv, const AdamHyper* __restrict__ hd) {
    AdamHyper h;
    if constexpr (DEV) h = *hd; else h = hv;
    // tensor of this chunk: binary search over <= 64 prefix entries (scalar registers: blockIdx is uniform)
    int lo = 0, hi = pk.count;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if ((int)blockIdx.x >= pk.first[mid]) lo = mid; else hi = mid; }
    const int ti = lo;
    const int64_t n = pk.n[ti];
    float* __restrict__ p = pk.p[ti]; float* __restrict__ g = pk.g[ti];
    float* __restrict__ m = pk.m[ti]; float* __restrict__ v = pk.v[ti];
    bf16_t* __restrict__ sh = pk.shadow[ti];
    const int64_t e0 = (int64_t)((int)blockIdx.x - pk.first[ti]) * ADAM_CHUNK;
    const int64_t e1 = e0 + ADAM_CHUNK < n ? e0 + ADAM_CHUNK : n;
    const bool vec = ((((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v) & 15) == 0) && (sh == nullptr || (((uintptr_t)sh) & 7) == 0);
    if (vec && e1 - e0 == ADAM_CHUNK) {
        // full chunk: four passes of 4 float4 per stream and thread, the sixteen loads of a pass issued before its first use
#pragma unroll 1
        for (int pass = 0; pass < ADAM_CHUNK / 4096; ++pass) {
        const int64_t i0 = e0 / 4 + pass * 1024 + threadIdx.x;
        float4 P[4], G[4], M[4], V[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) { P[u] = ldg_stream(p + 4 * (i0 + 256 * u)); G[u] = ldg_stream(g + 4 * (i0 + 256 * u)); }
#pragma unroll
        for (int u = 0; u < 4; ++u) { M[u] = ldg_stream(m + 4 * (i0 + 256 * u)); V[u] = ldg_stream(v + 4 * (i0 + 256 * u)); }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int64_t i = i0 + 256 * u;
            adam_one(P[u].x, G[u].x, M[u].x, V[u].x, h); adam_one(P[u].y, G[u].y, M[u].y, V[u].y, h);
            adam_one(P[u].z, G[u].z, M[u].z, V[u].z, h); adam_one(P[u].w, G[u].w, M[u].w, V[u].w, h);
            stg_stream(p + 4 * i, P[u]); stg_stream(m + 4 * i, M[u]); stg_stream(v + 4 * i, V[u]);
            if (h.mutate_grad) stg_stream(g + 4 * i, G[u]);
            if (sh) reinterpret_cast<uint2*>(sh)[i] = h.shadow_f16 ? make_uint2(pack_h2(P[u].x, P[u].y), pack_h2(P[u].z, P[u].w))
                                                                   : make_uint2(pack_bf2(P[u].x, P[u].y), pack_bf2(P[u].z, P[u].w));
        }
        }
        return;
    }
    // last chunk of a tensor / unaligned tensor: the vector part of what is left, then the scalar tail
    const int64_t nv = vec ? (e1 - e0) / 4 : 0;
    for (int64_t k = threadIdx.x; k < nv; k += 256) {
        const int64_t i = e0 / 4 + k;
        float4 P = ldg_stream(p + 4 * i), G = ldg_stream(g + 4 * i), M = ldg_stream(m + 4 * i), V = ldg_stream(v + 4 * i);
        adam_one(P.x, G.x, M.x, V.x, h); adam_one(P.y, G.y, M.y, V.y, h);
        adam_one(P.z, G.z, M.z, V.z, h); adam_one(P.w, G.w, M.w, V.w, h);
        stg_stream(p + 4 * i, P); stg_stream(m + 4 * i, M); stg_stream(v + 4 * i, V);
        if (h.mutate_grad) stg_stream(g + 4 * i, G);
        if (sh) reinterpret_cast<uint2*>(sh)[i] = h.shadow_f16 ? make_uint2(pack_h2(P.x, P.y), pack_h2(P.z, P.w)) : make_uint2(pack_bf2(P.x, P.y), pack_bf2(P.z, P.w));
    }
    for (int64_t i = e0 + nv * 4 + threadIdx.x; i < e1; i += 256) {
        float P = p[i], G = g[i], M = m[i], V = v[i];
        adam_one(P, G, M, V, h);
        p[i] = P; m[i] = M; v[i] = V;
        if (h.mutate_grad) g[i] = G;
        if (sh) sh[i] = h.shadow_f16 ? f2h(P).v : f2bf(P);
    }
}
static int adamw_form() {                                   // CTMI_ADAMW_FLAT=0: the (stride loop, tensor) grid of rounds 1-5, for A/B runs
    static const int f = ctmi_env_int("CTMI_ADAMW_FLAT", 1);
    return f;
}

static int mt_grid_x(const int64_t* n, int count) {
    int64_t mx = 1;
    for (int i = 0; i < count; ++i) mx = std::max(mx, n[i]);
    return (int)std::min<int64_t>(cdiv64(mx, 256 * 4 * 4), 2048);
}

// Walks `count` tensors in packs of CTMI_MT_MAX: fills an MTPack from the pointer arrays (an absent array gives nullptr entries) and hands it,
// with its (stride loop, tensor) grid, to `launch`.  `who` != nullptr: an entry of a given array that is null, or a negative size, is
// "<who>: null tensor %d" (checked pack by pack, as the launches go).
template <typename L>
static int mt_for_packs(float* const* p, float* const* g, float* const* m, float* const* v, void* const* shadow, const int64_t* n, int count,
                        const char* who, L&& launch) {
    for (int base = 0; base < count; base += CTMI_MT_MAX) {
        const int c = std::min(CTMI_MT_MAX, count - base);
        MTPack pk;
        for (int i = 0; i < c; ++i) {
            const int k = base + i;
            if (who) CTMI_REQUIRE((!p || p[k]) && (!g || g[k]) && (!m || m[k]) && (!v || v[k]) && n[k] >= 0, "%s: null tensor %d", who, k);
            pk.p[i] = p ? p[k] : nullptr; pk.g[i] = g ? g[k] : nullptr; pk.m[i] = m ? m[k] : nullptr; pk.v[i] = v ? v[k] : nullptr;
            pk.shadow[i] = shadow ? (bf16_t*)shadow[k] : nullptr; pk.n[i] = n[k];
        }
        const int rc = launch(pk, dim3(mt_grid_x(n + base, c), c));
        if (rc != CTMI_OK) return rc;
    }
    return CTMI_OK;
}

static AdamHyper adam_hyper(float lr, float beta1, float beta2, float eps, float weight_decay, int step, int decoupled, int mutate_grad, float grad_scale) {
    AdamHyper h;
    h.lr = lr; h.b1 = beta1; h.b2 = beta2; h.eps = eps; h.wd = weight_decay;
    const double bc1 = 1.0 - pow((double)beta1, (double)step), bc2 = 1.0 - pow((double)beta2, (double)step);
    h.bc1 = (float)bc1; h.bc2 = (float)bc2; h.sqrt_bc2 = (float)sqrt(bc2);
    h.shadow_f16 = (mutate_grad & CTMI_OPT_SHADOW_F16) ? 1 : 0;
    mutate_grad &= 1;
    h.gscale = grad_scale; h.decoupled = decoupled; h.mutate_grad = (mutate_grad && !decoupled && weight_decay != 0.f) || (mutate_grad && grad_scale != 1.0f);
    return h;
}
__global__ void adam_set_hyper_k(AdamHyper h, AdamHyper* dst) { if (threadIdx.x == 0 && blockIdx.x == 0) *dst = h; }

// one launch per <= CTMI_MT_FLAT tensors; hd != nullptr: the hyper-parameters come from the device record
static int adamw_flat_launch(float* const* p, float* const* g, float* const* m, float* const* v, void* const* shadow, const int64_t* n, int count,
                             const AdamHyper& h, const AdamHyper* hd, hipStream_t st) {
        for (int base = 0; base < count; ) {
            MTFlat pk;
            int c = 0;
            int64_t chunks = 0;
            while (base + c < count && c < CTMI_MT_FLAT) {
                const int i = base + c;
                CTMI_REQUIRE(p[i] && g[i] && m[i] && v[i] && n[i] >= 0, "adamw_step: null tensor %d", i);
                const int64_t ch = cdiv64(n[i], ADAM_CHUNK);
                if (chunks + ch > (int64_t)0x7fffffff) break;                       // (a launch's grid; never reached below 3.5e13 elements)
                pk.p[c] = p[i]; pk.g[c] = g[i]; pk.m[c] = m[i]; pk.v[c] = v[i];
                pk.shadow[c] = shadow ? (bf16_t*)shadow[i] : nullptr; pk.n[c] = n[i];
                pk.first[c] = (int)chunks;
                chunks += ch;
                ++c;
            }
            CTMI_REQUIRE(c > 0, "adamw_step: tensor %d is too large for one launch", base);
            pk.first[c] = (int)chunks; pk.count = c;
            for (int i = c; i < CTMI_MT_FLAT; ++i) { pk.p[i] = pk.g[i] = pk.m[i] = pk.v[i] = nullptr; pk.shadow[i] = nullptr; pk.n[i] = 0; pk.first[i + 1] = (int)chunks; }
            if (chunks > 0) {
                if (hd != nullptr) hipLaunchKernelGGL(adamw_flat_k<true>, dim3((unsigned)chunks), dim3(256), 0, st, pk, h, hd);
                else hipLaunchKernelGGL(adamw_flat_k<false>, dim3((unsigned)chunks), dim3(256), 0, st, pk, h, hd);
                CTMI_CHECK_LAUNCH("adamw_step");
            }
            base += c;
        }
        return CTMI_OK;
}

extern "C" int ctmi_adamw_set_hyper(void* hyper_dev, float lr, float beta1, float beta2, float eps, float weight_decay, int step, int decoupled,
                                    int mutate_grad, float grad_scale, void* stream) {
    CTMI_REQUIRE(hyper_dev != nullptr && step >= 1 && (((uintptr_t)hyper_dev) & 3) == 0, "adamw_set_hyper: bad args (step must be >= 1)");
    const AdamHyper h = adam_hyper(lr, beta1, beta2, eps, weight_decay, step, decoupled, mutate_grad, grad_scale);
    hipLaunchKernelGGL(adam_set_hyper_k, dim3(1), dim3(64), 0, as_stream(stream), h, reinterpret_cast<AdamHyper*>(hyper_dev));
    CTMI_CHECK_LAUNCH("adamw_set_hyper");
    return CTMI_OK;
}
extern "C" int ctmi_adamw_step_dev(float* const* p, float* const* g, float* const* m, float* const* v, void* const* shadow,
                                   const int64_t* n, int count, const void* hyper_dev, void* stream) {
    ProfScope prof__(CTMI_PROF_OPTIMIZER, as_stream(stream));
    CTMI_REQUIRE(p && g && m && v && n && count >= 0 && hyper_dev != nullptr, "adamw_step_dev: bad args");
    const AdamHyper unused = {};
    return adamw_flat_launch(p, g, m, v, shadow, n, count, unused, reinterpret_cast<const AdamHyper*>(hyper_dev), as_stream(stream));
}

extern "C" int ctmi_adamw_step(float* const* p, float* const* g, float* const* m, float* const* v, void* const* shadow,
                               const int64_t* n, int count, float lr, float beta1, float beta2, float eps,
                               float weight_decay, int step, int decoupled, int mutate_grad, float grad_scale, void* stream) {
    ProfScope prof__(CTMI_PROF_OPTIMIZER, as_stream(stream));
    CTMI_REQUIRE(p && g && m && v && n && count >= 0 && step >= 1, "adamw_step: bad args (step must be >= 1)");
    const bool legacy_grid = (mutate_grad & CTMI_OPT_LEGACY_GRID) != 0;
    const AdamHyper h = adam_hyper(lr, beta1, beta2, eps, weight_decay, step, decoupled, mutate_grad, grad_scale);
    if (adamw_form() != 0 && !legacy_grid) return adamw_flat_launch(p, g, m, v, shadow, n, count, h, nullptr, as_stream(stream));
    return mt_for_packs(p, g, m, v, shadow, n, count, "adamw_step", [&](const MTPack& pk, dim3 grid) -> int {
        hipLaunchKernelGGL(adamw_mt_k, grid, dim3(256), 0, as_stream(stream), pk, h);
        CTMI_CHECK_LAUNCH("adamw_step");
        return CTMI_OK;
    });
}

// ------------------------------------------------------------------------------------------------ loss scaling (GradScaler)
// torch.cuda.amp.GradScaler semantics (ft_bloom_DDP.py:107-128: scaler.scale(loss).backward(); scaler.step(opt); scaler.update()).
// state[0] = scale, state[1] = growth tracker, state[2] = found_inf (0/1) — one device-resident record, so scale() / unscale /
// update never read the scale on the host.  Unscale is in place (the caller can inspect true gradients after step(), as with
// torch) and multi-tensor: one launch per <= 24 gradients instead of one per parameter.
__global__ __launch_bounds__(256) void amp_unscale_k(MTPack pk, float* __restrict__ state) {
    const int ti = blockIdx.y;
    const int64_t n = pk.n[ti];
    float* __restrict__ g = pk.g[ti];
    const float inv = 1.0f / state[0];
    bool bad = false;
    const bool vec = (((uintptr_t)g) & 15) == 0;
    const int64_t n4 = vec ? n / 4 : 0;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
        float4 G = reinterpret_cast<float4*>(g)[i];
        G.x *= inv; G.y *= inv; G.z *= inv; G.w *= inv;
        bad |= !(isfinite(G.x) && isfinite(G.y) && isfinite(G.z) && isfinite(G.w));
        reinterpret_cast<float4*>(g)[i] = G;
    }
    for (int64_t i = n4 * 4 + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride) {
        const float G = g[i] * inv;
        bad |= !isfinite(G);
        g[i] = G;
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) state[2] = 1.0f;          // benign race: every writer stores the same value
}
extern "C" int ctmi_amp_unscale(float* const* g, const int64_t* n, int count, float* state, void* stream) {
    ProfScope prof__(CTMI_PROF_OPTIMIZER, as_stream(stream));
    CTMI_REQUIRE(g && n && state && count >= 0, "amp_unscale: bad args");
    return mt_for_packs(nullptr, g, nullptr, nullptr, nullptr, n, count, "amp_unscale", [&](const MTPack& pk, dim3 grid) -> int {
        hipLaunchKernelGGL(amp_unscale_k, grid, dim3(256), 0, as_stream(stream), pk, state);
        CTMI_CHECK_LAUNCH("amp_unscale");
        return CTMI_OK;
    });
}
// torch's _amp_update_scale_: found_inf -> scale *= backoff, tracker = 0; else ++tracker, and at growth_interval scale *= growth
// (only if the grown scale is finite), tracker = 0.  Clears found_inf for the next step.
__global__ void amp_update_k(float* __restrict__ state, float growth, float backoff, int interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (state[2] != 0.0f) { state[0] *= backoff; state[1] = 0.0f; }
    else {
        const float t = state[1] + 1.0f;
        if ((int)t == interval) { const float ns = state[0] * growth; if (isfinite(ns)) state[0] = ns; state[1] = 0.0f; }
        else state[1] = t;
    }
    state[2] = 0.0f;
}
extern "C" int ctmi_amp_update(float* state, float growth, float backoff, int interval, void* stream) {
    ProfScope prof__(CTMI_PROF_OPTIMIZER, as_stream(stream));
    CTMI_REQUIRE(state && interval >= 1, "amp_update: bad args");
    hipLaunchKernelGGL(amp_update_k, dim3(1), dim3(64), 0, as_stream(stream), state, growth, backoff, interval);
    CTMI_CHECK_LAUNCH("amp_update");
    return CTMI_OK;
}

struct SgdHyper { float lr, momentum, dampening, wd; int first, shadow_f16; };
__global__ __launch_bounds__(256) void sgd_mt_k(MTPack pk, SgdHyper h) {
    const int ti = blockIdx.y;
    const int64_t n = pk.n[ti];
    float* __restrict__ p = pk.p[ti]; float* __restrict__ g = pk.g[ti]; float* __restrict__ buf = pk.m[ti];
    bf16_t* __restrict__ sh = pk.shadow[ti];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        float P = p[i], G = g[i];
        if (h.wd != 0.f) G += h.wd * P;                         // optimizer.py:38-39
        if (buf != nullptr) {                                    // optimizer.py:41-48
            float B = h.first ? G : h.momentum * buf[i] + (1.0f - h.dampening) * G;
            buf[i] = B; G = B;
        }
        g[i] = G;                                                // the reference leaves param.grad = buf / decayed grad
        P -= h.lr * G;
        p[i] = P;
        if (sh) sh[i] = h.shadow_f16 ? f2h(P).v : f2bf(P);
    }
}
extern "C" int ctmi_sgd_step(float* const* p, float* const* g, float* const* buf, void* const* shadow, const int64_t* n,
                             int count, float lr, float momentum, float dampening, float weight_decay, int first_step, void* stream) {
    ProfScope prof__(CTMI_PROF_OPTIMIZER, as_stream(stream));
    CTMI_REQUIRE(p && g && n && count >= 0, "sgd_step: bad args");
    SgdHyper h{lr, momentum, dampening, weight_decay, first_step & 1, (first_step & CTMI_OPT_SHADOW_F16) ? 1 : 0};
    return mt_for_packs(p, g, buf, nullptr, shadow, n, count, nullptr, [&](const MTPack& pk, dim3 grid) -> int {
        hipLaunchKernelGGL(sgd_mt_k, grid, dim3(256), 0, as_stream(stream), pk, h);
        CTMI_CHECK_LAUNCH("sgd_step");
        return CTMI_OK;
    });
}

// ------------------------------------------------------------------------------------------------
// utilities
// ------------------------------------------------------------------------------------------------
template <typename S, typename D>
__global__ __launch_bounds__(256) void cast_k(const S* __restrict__ src, D* __restrict__ dst, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        dst[i] = Cvt<D>::from_f(Cvt<S>::to_f(src[i]));
}
__global__ __launch_bounds__(256) void cast_f32_bf16_v4(const float4* __restrict__ src, uint2* __restrict__ dst, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const float4 a = src[i];
        dst[i] = make_uint2(pack_bf2(a.x, a.y), pack_bf2(a.z, a.w));
    }
}
extern "C" int ctmi_cast(const void* src, int sd, void* dst, int dd, int64_t n, void* stream) {
    ProfScope prof__(CTMI_PROF_OTHER, as_stream(stream));
    CTMI_REQUIRE(src && dst && n >= 0, "cast: bad args");
    if (n == 0) return CTMI_OK;
    hipStream_t st = as_stream(stream);
    int grid = (int)std::min<int64_t>(cdiv64(n, 256 * 4), 4096);
    if (sd == CTMI_F32 && dd == CTMI_BF16 && aligned16(src) && ((((uintptr_t)dst) & 7) == 0) && n % 4 == 0) {
        hipLaunchKernelGGL(cast_f32_bf16_v4, dim3(grid), dim3(256), 0, st, (const float4*)src, (uint2*)dst, n / 4);
        CTMI_CHECK_LAUNCH("cast");
        return CTMI_OK;
    }
    const int rc = ctmi_by_dtype(sd, "cast", [&](auto s_) -> int { return ctmi_by_dtype(dd, "cast", [&](auto d_) -> int {
        using S = decltype(s_); using D = decltype(d_);
        if constexpr (std::is_same<S, D>::value || std::is_same<S, float>::value || std::is_same<D, float>::value) {
            hipLaunchKernelGGL((cast_k<S, D>), dim3(grid), dim3(256), 0, st, (const S*)src, (D*)dst, n);
            CTMI_CHECK_LAUNCH("cast");
            return CTMI_OK;
        } else return CTMI_ERR_UNSUPPORTED;                               // bf16 <-> fp16: no such kernel
    }); });
    if (rc == CTMI_ERR_UNSUPPORTED) ctmi_set_error("cast: unsupported dtypes %d->%d", sd, dd);
    return rc;
}

// dst[c][r] = (TD) src[r][c]   (src fp32 [R,C] row-major -> dst [C,R]): 64x64 tiles through padded LDS, coalesced both ways.
// GPT-2's Conv1D keeps its weight as [in,out] (modeling_gpt.py:32-46); the GEMM kernels read the [out,in] compute copy.
template <typename TD>
__global__ __launch_bounds__(256) void transpose_cast_k(const float* __restrict__ src, TD* __restrict__ dst, int64_t R, int64_t C) {
    __shared__ float tile[64][65];
    const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int64_t r = r0 + i, c = c0 + tx;
        tile[i][tx] = (r < R && c < C) ? src[r * C + c] : 0.f;
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int64_t c = c0 + i, r = r0 + tx;
        if (c < C && r < R) dst[c * R + r] = Cvt<TD>::from_f(tile[tx][i]);
    }
}
extern "C" int ctmi_transpose_cast(const float* src, void* dst, int dst_dtype, int64_t rows, int64_t cols, void* stream) {
    ProfScope prof__(CTMI_PROF_OTHER, as_stream(stream));
    CTMI_REQUIRE(src && dst && rows > 0 && cols > 0, "transpose_cast: bad args");
    const dim3 grid((unsigned)cdiv64(cols, 64), (unsigned)cdiv64(rows, 64));
    return ctmi_by_dtype(dst_dtype, "transpose_cast", [&](auto t) -> int {
        using TD = decltype(t);
        hipLaunchKernelGGL((transpose_cast_k<TD>), grid, dim3(256), 0, as_stream(stream), src, (TD*)dst, rows, cols);
        CTMI_CHECK_LAUNCH("transpose_cast");
        return CTMI_OK;
    });
}

__global__ __launch_bounds__(256) void sumsq_k(const float* __restrict__ x, int64_t n, double* __restrict__ out) {
    double s = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) { const double v = x[i]; s += v * v; }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    __shared__ double sm[4];
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd(out, sm[0] + sm[1] + sm[2] + sm[3]);
}
extern "C" int ctmi_sumsq(const float* x, int64_t n, double* out, int accumulate, void* stream) {
    ProfScope prof__(CTMI_PROF_OTHER, as_stream(stream));
    CTMI_REQUIRE(out && n >= 0 && (x || n == 0), "sumsq: bad args");      // an empty torch tensor has a null data pointer
    hipStream_t st = as_stream(stream);
    if (!accumulate) { if (hipMemsetAsync(out, 0, sizeof(double), st) != hipSuccess) { ctmi_set_error("sumsq: memset failed"); return CTMI_ERR_LAUNCH; } }
    if (n == 0) return CTMI_OK;
    int grid = (int)std::min<int64_t>(cdiv64(n, 256 * 8), 1024);
    hipLaunchKernelGGL(sumsq_k, dim3(grid), dim3(256), 0, st, x, n, out);
    CTMI_CHECK_LAUNCH("sumsq");
    return CTMI_OK;
}

// dst[i] = f * src[i]  (dst may alias src).  float4 body when both pointers are 16-byte aligned, scalar tail.
__global__ __launch_bounds__(256) void scale_copy_k(const float* src, float* dst, int64_t n, float s, const float* __restrict__ sd, int vec) {
    const float f = sd ? s * sd[0] : s;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nth = (int64_t)gridDim.x * 256;
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t i = tid; i < n4; i += nth) {
        float4 v = reinterpret_cast<const float4*>(src)[i];
        v.x *= f; v.y *= f; v.z *= f; v.w *= f;
        reinterpret_cast<float4*>(dst)[i] = v;
    }
    for (int64_t i = n4 * 4 + tid; i < n; i += nth) dst[i] = f * src[i];
}
static int scale_copy_launch(const float* src, float* dst, int64_t n, float s, const float* s_dev, void* stream, const char* what) {
    if (n == 0) return CTMI_OK;
    const int vec = ((((uintptr_t)src) | ((uintptr_t)dst)) & 15) == 0;
    int grid = (int)std::min<int64_t>(cdiv64(n, 256 * 16), 4096);
    hipLaunchKernelGGL(scale_copy_k, dim3(grid), dim3(256), 0, as_stream(stream), src, dst, n, s, s_dev, vec);
    CTMI_CHECK_LAUNCH(what);
    return CTMI_OK;
}
extern "C" int ctmi_scale(float* x, int64_t n, float s, const float* s_dev, void* stream) {
    ProfScope prof__(CTMI_PROF_OTHER, as_stream(stream));
    CTMI_REQUIRE(x && n >= 0, "scale: bad args");
    return scale_copy_launch(x, x, n, s, s_dev, stream, "scale");
}
extern "C" int ctmi_scale_copy(const float* src, float* dst, int64_t n, float s, void* stream) {
    ProfScope prof__(CTMI_PROF_OTHER, as_stream(stream));
    CTMI_REQUIRE(src && dst && n >= 0, "scale_copy: bad args");
    return scale_copy_launch(src, dst, n, s, nullptr, stream, "scale_copy");
}
