// DDIM inversion and latent interpolation (Song et al. 2020, §4.3, §5.3, eq. 67): the deterministic sampler run the other way, and the
// spherical interpolation of two latents.  Both entries are fp32, use static LDS only and no atomics, allocate nothing and call no
// attribute setter: a first call may sit inside a stream capture.  Driven by ddim.py (DDIM.encode / ddim.slerp).
#include "common.h"
#include "../../include/ddpm_hip.h"

// Every product and sum below is rounded on its own unless the code says fma: with the compiler free to contract, the 16-byte and the
// element-wise path of one kernel came out with different bits.  (Plain operators, not __fmul_rn / __fadd_rn: those are inline functions
// of the HIP headers, compiled under the command line's contraction mode whatever the pragma here says.)
#pragma clang fp contract(off)

namespace {

// ------------------------------------------------------------------------------------------------------------------ encode step
// x_next = cx[t] x + ce[t] eps, pred_x0 = r[t] x - rm1[t] eps: two products and one sum each, rounded separately (no contraction), so the
// result is that of the same three fp32 operations written in any other language.
struct EncodeTables { const float *cx, *ce, *recip, *recip_m1; };

// grid = (column blocks, B).  A sample whose four row bases are 16-byte aligned moves 16 bytes per lane over its first n / 4 * 4
// elements and finishes with a scalar tail; any other sample is scalar throughout.  x_next may be x: an element is read, then written,
// by the same lane.
__global__ __launch_bounds__(256) void ddim_encode_kernel(const float* x, const float* __restrict__ eps, const long long* __restrict__ t,
                                                          EncodeTables tb, float* x_next, float* __restrict__ pred_x0, int n, int S) {
    const long long base = (long long)blockIdx.y * n;
    const long long tt = t[blockIdx.y];
    const bool ok = (unsigned long long)tt < (unsigned long long)S;        // outside the tables: poison the sample, read nothing
    const float nan = __builtin_nanf("");
    const float cx = ok ? tb.cx[tt] : nan, ce = ok ? tb.ce[tt] : nan;
    const float r = ok ? tb.recip[tt] : nan, rm1 = ok ? tb.recip_m1[tt] : nan;
    const float* xb = x + base;
    const float* eb = eps + base;
    float* ob = x_next + base;
    float* pb = pred_x0 ? pred_x0 + base : nullptr;
    const bool vec = (((uintptr_t)xb | (uintptr_t)eb | (uintptr_t)ob | (uintptr_t)pb) & 15) == 0;
    const int nv = vec ? n >> 2 : 0;
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    for (int v = first; v < nv; v += stride) {
        f32x4 o = (f32x4)(nan), p = (f32x4)(nan);
        if (ok) {
            const f32x4 xv = reinterpret_cast<const f32x4*>(xb)[v], ev = reinterpret_cast<const f32x4*>(eb)[v];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = cx * xv[j] + ce * ev[j];
                p[j] = r * xv[j] - rm1 * ev[j];
            }
        }
        reinterpret_cast<f32x4*>(ob)[v] = o;
        if (pb) reinterpret_cast<f32x4*>(pb)[v] = p;
    }
    for (long long i = (long long)nv * 4 + first; i < n; i += stride) {
        float o = nan, p = nan;
        if (ok) {
            const float xv = xb[i], ev = eb[i];
            o = cx * xv + ce * ev;
            p = r * xv - rm1 * ev;
        }
        ob[i] = o;
        if (pb) pb[i] = p;
    }
}

// ------------------------------------------------------------------------------------------------------------------ slerp
// A pair is cut into chunks of SLERP_CHUNK elements, one workgroup each in both passes, so a pair is spread over n / SLERP_CHUNK
// workgroups.  Pass one leaves (<a,b>, |a|^2, |b|^2) of every chunk in ws[pair][chunk][3][hi, lo]; pass two adds a pair's chunks up in double,
// in an order that depends on nothing but the chunk count, and forms the weights in double.  Every sum has a fixed order.
constexpr int SLERP_CHUNK = 2048;                  // elements per workgroup: 256 lanes x 2 x 16 bytes (or x 8 scalars)
constexpr int SLERP_PER_LANE = SLERP_CHUNK / 256;
constexpr int SLERP_KTILE = 64;                    // alphas whose weights sit in LDS at a time

static inline long long slerp_chunks(long long n) { return (n + SLERP_CHUNK - 1) / SLERP_CHUNK; }

// the chunk's elements of one operand into registers: lane l holds vectors l and l + 256 (VEC) or scalars l + 256 j; out of range = 0
template <bool VEC> __device__ __forceinline__ void slerp_load(const float* __restrict__ p, long long c0, long long n, float* r) {
    if (VEC) {
#pragma unroll
        for (int j = 0; j < SLERP_PER_LANE / 4; ++j) {
            const long long i = c0 + ((long long)j * 256 + threadIdx.x) * 4;
            const f32x4 v = i < n ? *reinterpret_cast<const f32x4*>(p + i) : (f32x4)(0.f);      // n % 4 == 0: a vector is in or out as a whole
            r[4 * j] = v.x; r[4 * j + 1] = v.y; r[4 * j + 2] = v.z; r[4 * j + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < SLERP_PER_LANE; ++j) {
            const long long i = c0 + j * 256 + threadIdx.x;
            r[j] = i < n ? p[i] : 0.f;
        }
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// The three sums of a chunk are formed in double (a product of two floats is exact there) and leave as (hi, lo) float pairs: the cosine
// of a pair is then good to ~1e-14, which keeps the weights of a nearly antiparallel pair (1 / sin(th) large) as exact as fp32 outputs allow.
template <bool VEC> __global__ __launch_bounds__(256) void slerp_partial_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                                float* __restrict__ ws, long long n) {
    __shared__ double part[4][3];
    const long long chunks = gridDim.x, c0 = (long long)blockIdx.x * SLERP_CHUNK, base = (long long)blockIdx.y * n;
    float ra[SLERP_PER_LANE], rb[SLERP_PER_LANE];
    slerp_load<VEC>(a + base, c0, n, ra);
    slerp_load<VEC>(b + base, c0, n, rb);
    double ab = 0.0, aa = 0.0, bb = 0.0;
#pragma unroll
    for (int j = 0; j < SLERP_PER_LANE; ++j) {
        const double x = (double)ra[j], y = (double)rb[j];
        ab = fma(x, y, ab);
        aa = fma(x, x, aa);
        bb = fma(y, y, bb);
    }
    ab = wave_sum_f64(ab); aa = wave_sum_f64(aa); bb = wave_sum_f64(bb);
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = ab; part[threadIdx.x >> 6][1] = aa; part[threadIdx.x >> 6][2] = bb; }
    __syncthreads();
    if (threadIdx.x < 3) {
        const int q = threadIdx.x;
        const double s = ((part[0][q] + part[1][q]) + part[2][q]) + part[3][q];
        const float hi = (float)s;                                          // inf / NaN: lo is NaN too, and so is the pair's cosine
        float* w = ws + (((long long)blockIdx.y * chunks + blockIdx.x) * 3 + q) * 2;
        w[0] = hi;
        w[1] = (float)(s - (double)hi);
    }
}

template <bool VEC> __global__ __launch_bounds__(256) void slerp_apply_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                              const float* __restrict__ alpha, const float* __restrict__ ws,
                                                                              float* __restrict__ out, int K, long long n) {
    __shared__ double tot[256][3];
    __shared__ float w[SLERP_KTILE][2];
    const long long chunks = gridDim.x, c0 = (long long)blockIdx.x * SLERP_CHUNK, base = (long long)blockIdx.y * n;
    // every workgroup of the pair adds the pair's chunks up itself, all in the same order: lane l takes chunks l, l + 256, ... and a
    // binary tree over the 256 lanes follows
    double s[3] = {0.0, 0.0, 0.0};
    const float* wp = ws + (long long)blockIdx.y * chunks * 6;
    for (long long c = threadIdx.x; c < chunks; c += 256)
#pragma unroll
        for (int q = 0; q < 3; ++q) s[q] += (double)wp[(c * 3 + q) * 2] + (double)wp[(c * 3 + q) * 2 + 1];
#pragma unroll
    for (int q = 0; q < 3; ++q) tot[threadIdx.x][q] = s[q];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (threadIdx.x < h)
#pragma unroll
            for (int q = 0; q < 3; ++q) tot[threadIdx.x][q] += tot[threadIdx.x + h][q];
        __syncthreads();
    }
    const double cs0 = tot[0][0] / (sqrt(tot[0][1]) * sqrt(tot[0][2]));
    const double cs = fmin(fmax(cs0, -1.0), 1.0);                           // NaN stays NaN
    const bool linear = !(1.0 - fabs(cs) >= 1e-6);                          // nearly (anti)parallel, or not finite (0 / 0, inf / inf, NaN)
    const double th = acos(cs), inv = 1.0 / sin(th);

    float ra[SLERP_PER_LANE], rb[SLERP_PER_LANE];
    slerp_load<VEC>(a + base, c0, n, ra);
    slerp_load<VEC>(b + base, c0, n, rb);
    for (int k0 = 0; k0 < K; k0 += SLERP_KTILE) {
        const int kt = min(SLERP_KTILE, K - k0);
        __syncthreads();                                                    // the previous tile's weights have been read
        if ((int)threadIdx.x < kt) {
            const double al = (double)alpha[k0 + threadIdx.x];
            w[threadIdx.x][0] = (float)(linear ? 1.0 - al : sin((1.0 - al) * th) * inv);
            w[threadIdx.x][1] = (float)(linear ? al : sin(al * th) * inv);
        }
        __syncthreads();
        for (int k = 0; k < kt; ++k) {
            const float w0 = w[k][0], w1 = w[k][1];
            float* o = out + ((long long)blockIdx.y * K + k0 + k) * n;
            // out = fma(w0, a, w1 * b): two roundings; alpha = 0 returns a and alpha = 1 returns b exactly (for finite operands)
            if (VEC) {
#pragma unroll
                for (int j = 0; j < SLERP_PER_LANE / 4; ++j) {
                    const long long i = c0 + ((long long)j * 256 + threadIdx.x) * 4;
                    f32x4 v;
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = fmaf(w0, ra[4 * j + e], w1 * rb[4 * j + e]);
                    if (i < n) *reinterpret_cast<f32x4*>(o + i) = v;
                }
            } else {
#pragma unroll
                for (int j = 0; j < SLERP_PER_LANE; ++j) {
                    const long long i = c0 + j * 256 + threadIdx.x;
                    if (i < n) o[i] = fmaf(w0, ra[j], w1 * rb[j]);
                }
            }
        }
    }
}

inline bool aligned4(const void* p) { return (((uintptr_t)p) & 3) == 0; }

}  // namespace

extern "C" int ddpm_ddim_encode_step(const float* x, const float* model_out, const long long* t, const float* cx, const float* ce,
                                     const float* sqrt_recip_ab_prev, const float* sqrt_recip_m1_ab_prev, float* x_next, float* pred_x0,
                                     int B, int n, int S, void* stream) {
    if (!x || !model_out || !t || !cx || !ce || !sqrt_recip_ab_prev || !sqrt_recip_m1_ab_prev || !x_next) return DDPM_ERR_NULL;
    if (B <= 0 || B > 65535 || n <= 0 || S <= 0) return DDPM_ERR_SHAPE;
    if (!aligned4(x) || !aligned4(model_out) || !aligned4(x_next) || !aligned4(pred_x0) || (((uintptr_t)t) & 7)) return DDPM_ERR_ALIGN;
    EncodeTables tb{cx, ce, sqrt_recip_ab_prev, sqrt_recip_m1_ab_prev};
    const int gx = n <= 1024 ? 1 : (n / 1024 < 256 ? n / 1024 : 256);       // about one 16-byte vector per lane and trip
    hipLaunchKernelGGL(ddim_encode_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x, model_out, t, tb, x_next, pred_x0, n, S);
    return check_launch();
}

extern "C" long long ddpm_slerp_workspace_floats(int P, int n) {
    if (P < 0 || n < 0) return -1;
    return 6ll * P * slerp_chunks(n);
}

extern "C" int ddpm_slerp(const float* a, const float* b, const float* alpha, float* out, float* ws, int P, int K, int n, void* stream) {
    if (!a || !b || !alpha || !out || !ws) return DDPM_ERR_NULL;
    if (P <= 0 || P > 65535 || K <= 0 || n <= 0) return DDPM_ERR_SHAPE;
    if (!aligned4(a) || !aligned4(b) || !aligned4(alpha) || !aligned4(out) || !aligned4(ws)) return DDPM_ERR_ALIGN;
    const bool vec = n % 4 == 0 && aligned16(a) && aligned16(b) && aligned16(out);
    const dim3 grid((unsigned)slerp_chunks(n), P), block(256);
    if (vec) {
        hipLaunchKernelGGL(slerp_partial_kernel<true>, grid, block, 0, (hipStream_t)stream, a, b, ws, (long long)n);
        hipLaunchKernelGGL(slerp_apply_kernel<true>, grid, block, 0, (hipStream_t)stream, a, b, alpha, (const float*)ws, out, K, (long long)n);
    } else {
        hipLaunchKernelGGL(slerp_partial_kernel<false>, grid, block, 0, (hipStream_t)stream, a, b, ws, (long long)n);
        hipLaunchKernelGGL(slerp_apply_kernel<false>, grid, block, 0, (hipStream_t)stream, a, b, alpha, (const float*)ws, out, K, (long long)n);
    }
    return check_launch();
}
