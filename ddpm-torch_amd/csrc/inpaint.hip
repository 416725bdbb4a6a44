// Inpainting and image editing (RePaint: Lugmayr et al., CVPR 2022, Algorithm 1): the masked sampling step — the known region re-noised
// from the source image at the level the reverse step arrives at, the unknown region from the reverse step itself, blended by a mask that
// is broadcast over channels — and the forward jump that takes a state back up j levels before it is brought down again.  Both entries are
// fp32, use static LDS only and no atomics, allocate nothing and call no attribute setter: a first call may sit inside a stream capture.
// Driven by diffusion.py (GaussianDiffusion.inpaint; ddim.DDIM inherits it on its own tables).
#include "common.h"
#include "../../include/ddpm_hip.h"

// Every product and sum below is rounded on its own (see csrc/ddim.hip: plain operators under this pragma).  The two fused operations of
// the sampling update live in step_elem (common.h), spelled as fma, so an element the mask leaves to the reverse step carries the bits
// of ddpm_p_sample_step / ddpm_p_sample_step_lv.
#pragma clang fp contract(off)

namespace {

inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3) == 0; }
inline bool aligned8(const void* p) { return (((uintptr_t)p) & 7) == 0; }
inline int column_blocks(int n) { return n <= 1024 ? 1 : (n / 1024 < 256 ? n / 1024 : 256); }       // about one 16-byte vector per lane and trip

// ------------------------------------------------------------------------------------------------------------------ masked step
struct MaskedTables { const float *recip, *recip_m1, *coef1, *coef2, *lv_lo, *lv_hi, *ka, *kb; };

// per-sample constants: the step's coefficients, the noise mask, the variance policy of p_step_kernel (elementwise.hip) and the two
// re-noising coefficients of the level the step arrives at
struct MaskedRow {
    VlbCoef k;
    float noise_mask, mask_sd, lv_min, lv_max, ka, kb;
    int mean_type, clip, var_mode;
};

// one element: u = the reverse step, kn = ka x_known + kb e, out = u | kn | m kn + (1 - m) u.  The selects keep what the mask excludes out
// of the arithmetic: NaN under a mask of 0 (in x_known, e) or 1 (in x_t, model_out, z) does not reach the output.
__device__ __forceinline__ float masked_elem(const MaskedRow& r, float xt, float o, float v, float z, float xk, float e, float m) {
    float mask_sd = r.mask_sd;
    if (r.var_mode != 0) mask_sd = r.noise_mask * expf(0.5f * lv_logvar(r.var_mode, v, r.lv_min, r.lv_max));
    float u, x0;
    step_elem(r.k, r.mean_type, r.clip, xt, o, mask_sd, z, u, x0);
    const float kn = r.ka * xk + r.kb * e;
    const float rest = 1.0f - m;
    const float mix = m * kn + rest * u;
    return m == 0.0f ? u : (m == 1.0f ? kn : mix);
}

// grid = (column blocks, B).  Sample b reads x_t[b], its network row (mean half, and the v half in var_mode 1 | 2), z[b], x_known[b],
// e[b] and its mask row, and writes x_prev[b].  A sample all of whose row bases are 16-byte aligned, with hw % 4 == 0 (then n % 4 == 0
// and a vector never straddles a mask row), moves 16 bytes per lane; any other sample is scalar throughout.  x_prev may be x_t: an
// element is read, then written, by the same lane.
__global__ __launch_bounds__(256) void p_step_masked_kernel(const float* x_t, const float* __restrict__ out, const float* __restrict__ z,
                                                            const float* __restrict__ x_known, const float* __restrict__ e,
                                                            const float* __restrict__ mask, const long long* __restrict__ t, MaskedTables tb,
                                                            float* x_prev, int n, int hw, int mask_rows, long long pitch, int mean_type,
                                                            int clip, int var_mode, int T) {
    const long long base = (long long)blockIdx.y * n;
    const long long tt = t[blockIdx.y];
    const bool ok = (unsigned long long)tt < (unsigned long long)T;        // outside the tables: poison the sample, read nothing
    const float nan = __builtin_nanf("");
    MaskedRow r{VlbCoef{nan, nan, nan, nan, 0.f, 0.f}, nan, nan, 0.f, 0.f, nan, nan, mean_type, clip, var_mode};
    if (ok) {
        r.k = VlbCoef{tb.recip[tt], tb.recip_m1[tt], tb.coef1[tt], tb.coef2[tt], 0.f, 0.f};
        r.noise_mask = tt > 0 ? 1.f : 0.f;
        if (var_mode == 0) {
            const float sd = expf(0.5f * tb.lv_lo[tt]);
            r.mask_sd = r.noise_mask * sd;
        } else if (var_mode == 2) {
            r.lv_min = tb.lv_lo[tt];
            r.lv_max = tb.lv_hi[tt];
        }
        r.ka = tb.ka[tt];
        r.kb = tb.kb[tt];
    }
    const float* xb = x_t + base;
    const float* ob = out + (long long)blockIdx.y * pitch;
    const float* vb = var_mode != 0 ? ob + n : nullptr;
    const float* zb = z + base;
    const float* kb = x_known + base;
    const float* eb = e + base;
    const float* mb = mask + (mask_rows == 1 ? 0ll : (long long)blockIdx.y * hw);
    float* db = x_prev + base;
    const bool vec = (hw & 3) == 0 &&
                     (((uintptr_t)xb | (uintptr_t)ob | (uintptr_t)vb | (uintptr_t)zb | (uintptr_t)kb | (uintptr_t)eb | (uintptr_t)mb | (uintptr_t)db) & 15) == 0;
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    if (vec) {
        const int nv = n >> 2;
        for (int v = first; v < nv; v += stride) {
            f32x4 o = (f32x4)(nan);
            if (ok) {
                const f32x4 xv = reinterpret_cast<const f32x4*>(xb)[v], ov = reinterpret_cast<const f32x4*>(ob)[v];
                const f32x4 zv = reinterpret_cast<const f32x4*>(zb)[v], kv = reinterpret_cast<const f32x4*>(kb)[v];
                const f32x4 ev = reinterpret_cast<const f32x4*>(eb)[v];
                const f32x4 mv = *reinterpret_cast<const f32x4*>(mb + (v * 4) % hw);
                const f32x4 vv = vb ? reinterpret_cast<const f32x4*>(vb)[v] : (f32x4)(0.f);
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = masked_elem(r, xv[j], ov[j], vv[j], zv[j], kv[j], ev[j], mv[j]);
            }
            reinterpret_cast<f32x4*>(db)[v] = o;
        }
        return;
    }
    for (int i = first; i < n; i += stride) {
        float o = nan;
        if (ok) o = masked_elem(r, xb[i], ob[i], vb ? vb[i] : 0.f, zb[i], kb[i], eb[i], mb[i % hw]);
        db[i] = o;
    }
}

// ------------------------------------------------------------------------------------------------------------------ forward jump
// x_out = ja[t] x + jb[t] z: two products and a sum, each rounded.  grid = (column blocks, B); 16 bytes per lane over the first n / 4 * 4
// elements of a sample whose three row bases are 16-byte aligned, with a scalar tail; element-wise otherwise.  x_out may be x.
__global__ __launch_bounds__(256) void q_jump_kernel(const float* x, const float* __restrict__ z, const long long* __restrict__ t,
                                                     const float* __restrict__ ja, const float* __restrict__ jb, float* x_out, int n, int T) {
    const long long base = (long long)blockIdx.y * n;
    const long long tt = t[blockIdx.y];
    const bool ok = (unsigned long long)tt < (unsigned long long)T;
    const float nan = __builtin_nanf("");
    const float a = ok ? ja[tt] : nan, b = ok ? jb[tt] : nan;
    const float* xb = x + base;
    const float* zb = z + base;
    float* ob = x_out + base;
    const bool vec = (((uintptr_t)xb | (uintptr_t)zb | (uintptr_t)ob) & 15) == 0;
    const int nv = vec ? n >> 2 : 0;
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int v = first; v < nv; v += stride) {
        f32x4 o = (f32x4)(nan);
        if (ok) {
            const f32x4 xv = reinterpret_cast<const f32x4*>(xb)[v], zv = reinterpret_cast<const f32x4*>(zb)[v];
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = a * xv[j] + b * zv[j];
        }
        reinterpret_cast<f32x4*>(ob)[v] = o;
    }
    for (long long i = (long long)nv * 4 + first; i < n; i += stride) {
        float o = nan;
        if (ok) o = a * xb[i] + b * zb[i];
        ob[i] = o;
    }
}

}  // namespace

extern "C" int ddpm_p_sample_step_masked(const float* x_t, const float* model_out, const float* z, const float* x_known, const float* e,
                                         const float* mask, const long long* t, const float* sqrt_recip_ab, const float* sqrt_recip_m1_ab,
                                         const float* post_coef1, const float* post_coef2, const float* logvar_lo, const float* logvar_hi,
                                         const float* sqrt_ab_prev, const float* sqrt_1mab_prev, float* x_prev, int B, int n, int hw,
                                         int mask_rows, int out_pitch, int mean_type, int clip, int var_mode, int T, void* stream) {
    if (!x_t || !model_out || !z || !x_known || !e || !mask || !t || !sqrt_recip_ab || !sqrt_recip_m1_ab || !post_coef1 || !post_coef2 ||
        !sqrt_ab_prev || !sqrt_1mab_prev || !x_prev)
        return DDPM_ERR_NULL;
    if (B <= 0 || B > 65535 || n <= 0 || hw <= 0 || T <= 0 || n % hw != 0 || (mask_rows != 1 && mask_rows != B)) return DDPM_ERR_SHAPE;
    if ((out_pitch != n && (long long)out_pitch != 2ll * n) || mean_type < 0 || mean_type > 2 || var_mode < 0 || var_mode > 2) return DDPM_ERR_SHAPE;
    if (var_mode != 0 && (long long)out_pitch != 2ll * n) return DDPM_ERR_SHAPE;
    if ((var_mode != 1 && !logvar_lo) || (var_mode == 2 && !logvar_hi)) return DDPM_ERR_NULL;
    if (!aligned4(x_t) || !aligned4(model_out) || !aligned4(z) || !aligned4(x_known) || !aligned4(e) || !aligned4(mask) || !aligned4(x_prev) ||
        !aligned8(t))
        return DDPM_ERR_ALIGN;
    MaskedTables tb{sqrt_recip_ab, sqrt_recip_m1_ab, post_coef1, post_coef2, logvar_lo, logvar_hi, sqrt_ab_prev, sqrt_1mab_prev};
    hipLaunchKernelGGL(p_step_masked_kernel, dim3(column_blocks(n), B), dim3(256), 0, (hipStream_t)stream, x_t, model_out, z, x_known, e, mask, t,
                       tb, x_prev, n, hw, mask_rows, (long long)out_pitch, mean_type, clip, var_mode, T);
    return check_launch();
}

extern "C" int ddpm_q_jump(const float* x, const float* z, const long long* t, const float* ja, const float* jb, float* x_out, int B, int n,
                           int T, void* stream) {
    if (!x || !z || !t || !ja || !jb || !x_out) return DDPM_ERR_NULL;
    if (B <= 0 || B > 65535 || n <= 0 || T <= 0) return DDPM_ERR_SHAPE;
    if (!aligned4(x) || !aligned4(z) || !aligned4(x_out) || !aligned8(t)) return DDPM_ERR_ALIGN;
    hipLaunchKernelGGL(q_jump_kernel, dim3(column_blocks(n), B), dim3(256), 0, (hipStream_t)stream, x, z, t, ja, jb, x_out, n, T);
    return check_launch();
}
