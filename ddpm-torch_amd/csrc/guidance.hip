// Class conditioning and classifier-free guidance (Ho & Salimans 2022): the class-embedding add in front of the shared SiLU of the time path,
// its table gradient, and the guided sampling step on the network output of a doubled batch.  All three entries are fp32, use static LDS
// only and no atomics, allocate nothing and call no attribute setter: a first call may sit inside a stream capture.  Driven by
// models/unet.py (_Engine._time_biases / _temb_bwd) and diffusion.py (the guided form of the sampling step; ddim.py on its own tables).
#include "common.h"
#include "../../include/ddpm_hip.h"

// Every product and sum below is rounded on its own (see csrc/ddim.hip: plain operators under this pragma, not __fmul_rn / __fadd_rn, which
// the compiler contracts all the same).  The two fused operations of the sampling update live in step_elem (common.h), spelled as fma.
#pragma clang fp contract(off)

namespace {

inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3) == 0; }
inline bool aligned8(const void* p) { return (((uintptr_t)p) & 7) == 0; }
inline int flat_grid(long long n) { const long long g = (n + 255) / 256; return (int)(g < 1 ? 1 : (g > 4096 ? 4096 : g)); }

// ------------------------------------------------------------------------------------------------------------------ class embedding
// pre[b] = t_emb[b] + table[y[b]], s[b] = SiLU(pre[b]) with silu_fwd_kernel's expression (siluf_).  A label outside [0, K1) poisons the
// two rows of its sample and reads no table row.
__global__ __launch_bounds__(256) void class_embed_fwd_kernel(const float* __restrict__ t_emb, const float* __restrict__ table,
                                                              const long long* __restrict__ y, float* __restrict__ pre, float* __restrict__ s,
                                                              int B, int E, int K1) {
    const long long tot = (long long)B * E;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < tot; i += (long long)gridDim.x * 256) {
        const long long b = i / E, e = i - b * E;
        const long long k = y[b];
        float p = __builtin_nanf("");
        if ((unsigned long long)k < (unsigned long long)K1) p = t_emb[i] + table[k * E + e];
        pre[i] = p;
        s[i] = siluf_(p);
    }
}

// dtable[k][e] = sum of dpre[b][e] over the samples with y[b] == k, in ascending b.  grid = (column blocks, K1): a workgroup owns 256
// columns of one class, walks the batch in chunks of 256 labels (compared once, kept in LDS) and reads the matching rows alone.  Plain
// stores to every element: a class without a sample gets 0.0 whatever the buffer held.
__global__ __launch_bounds__(256) void class_embed_bwd_kernel(const float* __restrict__ dpre, const long long* __restrict__ y,
                                                              float* __restrict__ dtable, int B, int E) {
    __shared__ int hit[256];
    const long long k = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    float acc = 0.0f;
    for (int b0 = 0; b0 < B; b0 += 256) {
        const int b = b0 + threadIdx.x;
        hit[threadIdx.x] = b < B && y[b] == k;
        __syncthreads();
        const int m = min(256, B - b0);
        if (e < E)
            for (int j = 0; j < m; ++j)
                if (hit[j]) acc = acc + dpre[(long long)(b0 + j) * E + e];
        __syncthreads();                                                    // the chunk's flags have been read
    }
    if (e < E) dtable[k * E + e] = acc;
}

// ------------------------------------------------------------------------------------------------------------------ guided step
struct CfgTables { const float *recip, *recip_m1, *coef1, *coef2, *logvar; };

// one element: g = scale out_c + (1 - scale) out_u (two products and a sum, three roundings), then ddpm_p_sample_step's update on g
__device__ __forceinline__ void cfg_elem(const VlbCoef& k, float scale, float rest, int mean_type, int clip, float xt, float oc, float ou, float mask_sd,
                                         float z, float& x_prev, float& x0) {
    const float g = scale * oc + rest * ou;
    step_elem(k, mean_type, clip, xt, g, mask_sd, z, x_prev, x0);
}

// grid = (column blocks, B).  Sample b reads x_t[b], out2[b] (conditional), out2[B + b] (unconditional), z[b] and writes x_prev[b], with
// dup also x_prev[B + b], and pred_x0[b].  A sample all of whose row bases are 16-byte aligned moves 16 bytes per lane over its first
// n / 4 * 4 elements and ends with a scalar tail; any other sample is scalar throughout.  x_prev may be x_t: an element is read, then
// written, by the same lane, and rows [B, 2B) of x_t are never read.
__global__ __launch_bounds__(256) void p_step_cfg_kernel(const float* x_t, const float* __restrict__ out2, const float* __restrict__ z,
                                                         const long long* __restrict__ t, CfgTables tb, float scale, float* x_prev,
                                                         float* __restrict__ pred_x0, int n, int mean_type, int clip, int dup, int T) {
    const long long B = gridDim.y, base = (long long)blockIdx.y * n, base_u = ((long long)blockIdx.y + B) * n;
    const long long tt = t[blockIdx.y];
    const bool ok = (unsigned long long)tt < (unsigned long long)T;        // outside the tables: poison the sample, read nothing
    const float nan = __builtin_nanf("");
    VlbCoef k{nan, nan, nan, nan, 0.f, 0.f};
    float mask_sd = nan;
    if (ok) {
        k = VlbCoef{tb.recip[tt], tb.recip_m1[tt], tb.coef1[tt], tb.coef2[tt], 0.f, 0.f};
        const float mask = tt > 0 ? 1.f : 0.f;
        const float sd = expf(0.5f * tb.logvar[tt]);
        mask_sd = mask * sd;
    }
    const float rest = 1.0f - scale;
    const float* xb = x_t + base;
    const float* cb = out2 + base;
    const float* ub = out2 + base_u;
    const float* zb = z + base;
    float* ob = x_prev + base;
    float* db = dup ? x_prev + base_u : nullptr;
    float* pb = pred_x0 ? pred_x0 + base : nullptr;
    const bool vec = (((uintptr_t)xb | (uintptr_t)cb | (uintptr_t)ub | (uintptr_t)zb | (uintptr_t)ob | (uintptr_t)db | (uintptr_t)pb) & 15) == 0;
    const int nv = vec ? n >> 2 : 0;
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int v = first; v < nv; v += stride) {
        f32x4 o = (f32x4)(nan), p = (f32x4)(nan);
        if (ok) {
            const f32x4 xv = reinterpret_cast<const f32x4*>(xb)[v], cv = reinterpret_cast<const f32x4*>(cb)[v];
            const f32x4 uv = reinterpret_cast<const f32x4*>(ub)[v], zv = reinterpret_cast<const f32x4*>(zb)[v];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float xp, x0;
                cfg_elem(k, scale, rest, mean_type, clip, xv[j], cv[j], uv[j], mask_sd, zv[j], xp, x0);
                o[j] = xp; p[j] = x0;
            }
        }
        reinterpret_cast<f32x4*>(ob)[v] = o;
        if (db) reinterpret_cast<f32x4*>(db)[v] = o;
        if (pb) reinterpret_cast<f32x4*>(pb)[v] = p;
    }
    for (long long i = (long long)nv * 4 + first; i < n; i += stride) {
        float o = nan, p = nan;
        if (ok) cfg_elem(k, scale, rest, mean_type, clip, xb[i], cb[i], ub[i], mask_sd, zb[i], o, p);
        ob[i] = o;
        if (db) db[i] = o;
        if (pb) pb[i] = p;
    }
}

}  // namespace

extern "C" int ddpm_class_embed_fwd(const float* t_emb, const float* table, const long long* y, float* pre, float* s, int B, int E, int K1,
                                    void* stream) {
    if (!t_emb || !table || !y || !pre || !s) return DDPM_ERR_NULL;
    if (B <= 0 || E <= 0 || K1 <= 0) return DDPM_ERR_SHAPE;
    if (!aligned4(t_emb) || !aligned4(table) || !aligned4(pre) || !aligned4(s) || !aligned8(y)) return DDPM_ERR_ALIGN;
    hipLaunchKernelGGL(class_embed_fwd_kernel, dim3(flat_grid((long long)B * E)), dim3(256), 0, (hipStream_t)stream, t_emb, table, y, pre, s, B, E, K1);
    return check_launch();
}

extern "C" int ddpm_class_embed_bwd(const float* dpre, const long long* y, float* dtable, int B, int E, int K1, void* stream) {
    if (!dpre || !y || !dtable) return DDPM_ERR_NULL;
    if (B <= 0 || E <= 0 || K1 <= 0 || K1 > 65535) return DDPM_ERR_SHAPE;
    if (!aligned4(dpre) || !aligned4(dtable) || !aligned8(y)) return DDPM_ERR_ALIGN;
    hipLaunchKernelGGL(class_embed_bwd_kernel, dim3((E + 255) / 256, K1), dim3(256), 0, (hipStream_t)stream, dpre, y, dtable, B, E);
    return check_launch();
}

extern "C" int ddpm_p_sample_step_cfg(const float* x_t, const float* model_out2, const float* z, const long long* t,
                                      const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab, const float* post_coef1, const float* post_coef2,
                                      const float* logvar, float scale, float* x_prev, float* pred_x0, int B, int n, int mean_type, int clip,
                                      int dup, int T, void* stream) {
    if (!x_t || !model_out2 || !z || !t || !x_prev || !sqrt_recip_ab || !sqrt_recip_m1_ab || !post_coef1 || !post_coef2 || !logvar) return DDPM_ERR_NULL;
    if (B <= 0 || B > 65535 || n <= 0 || T <= 0 || mean_type < 0 || mean_type > 2) return DDPM_ERR_SHAPE;
    if (!aligned4(x_t) || !aligned4(model_out2) || !aligned4(z) || !aligned4(x_prev) || !aligned4(pred_x0) || !aligned8(t)) return DDPM_ERR_ALIGN;
    CfgTables tb{sqrt_recip_ab, sqrt_recip_m1_ab, post_coef1, post_coef2, logvar};
    const int gx = n <= 1024 ? 1 : (n / 1024 < 256 ? n / 1024 : 256);       // about one 16-byte vector per lane and trip
    hipLaunchKernelGGL(p_step_cfg_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x_t, model_out2, z, t, tb, scale, x_prev, pred_x0, n,
                       mean_type, clip, dup, T);
    return check_launch();
}
