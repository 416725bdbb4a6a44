// The 2-D toy denoiser (upstream toy/toy_model.py:17-62, BASELINE config 1) as gfx950 kernels, fp32 throughout.
//
//   Decoder(D, M, L):  h_0 = x W_in^T
//                      E[t] = enc(lrelu(t_proj(temb(t))))                      one [M] row per timestep: the time table
//                      h_{l+1} = h_l + fc2(lrelu(LN2(fc1(lrelu(LN1(h_l))) + E[t])))   the SAME layer object L times
//                      y = out_fc(LN_out(h_L))
//
// Forward: one workgroup per 32-row tile keeps the tile on chip from x to y (two [32][M] LDS images: the residual stream h and
// the layer's working row).  The M x M products run on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate: exact fp32 at the fp32 vector
// rate); each wave owns 32-column output tiles, the A operand comes from LDS and the weights from L1/L2 (128 KB at M = 128: every
// workgroup of the grid reads the same lines).  The k index inside an 8-wide step is permuted identically for A and B (lane half kh
// supplies k0 + 4 kh + j to MFMA j), so both operands load as 16-byte vectors.
//
// Backward: the same tiles recompute what the forward did not keep (only h_l and the LayerNorm (mean, rstd) are saved) and write the
// operands of the weight gradients of the shared layer — fc1: (dZ_l, A1_l), fc2: (dh_{l+1}, A2_l) — as [L*B][M] matrices; a split-K
// MFMA kernel sums dW = P^T Q over all L*B rows into per-split slabs and an ordered pass adds the slabs.  The small gradients
// (LayerNorms, in_fc, out_fc) leave each tile as a partial slab, added in tile order.  dE[t] (the fc1-input gradient of every row,
// summed over layers, then over the rows with that t) is gathered per timestep in row order.  No float atomics anywhere: a repeated
// backward is bit-identical.
#include "common.h"

#include <string.h>

namespace {

constexpr int RT = 32;           // rows per tile (the MFMA's M)
constexpr int NT = 256;          // threads per workgroup (4 waves)
constexpr int MAXD = 16;
constexpr float SLOPE = 0.02f;   // toy_model.py:14
constexpr float LN_EPS = 1e-5f;  // nn.LayerNorm default

struct ToyW {
    const float *win, *g1, *b1, *fc1, *g2, *b2, *fc2, *gon, *bon, *wout, *bout;
};

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : v * SLOPE; }
__device__ __forceinline__ float lrelu_grad(float pre, float g) { return pre > 0.f ? g : g * SLOPE; }

// acc (32 rows x 32 columns n0..n0+31) = A[32][M] (LDS, pitch P) x op(W):  op(W)[k][n] = W[n][k] (TRANS = false: x W^T, the forward of
// nn.Linear) or W[k][n] (TRANS = true: g W, its input gradient).  Result element v of lane l: row (v&3) + 8(v>>2) + 4(l>>5), column n0 + (l&31).
template <bool TRANS>
__device__ __forceinline__ void tile_gemm(const float* A, int P, const float* __restrict__ W, int M, int n0, f32x16& acc) {
    const int lane = threadIdx.x & 63, i = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    const float* ap = A + i * P + 4 * kh;

    for (int k0 = 0; k0 < M; k0 += 8) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(ap + k0);
        f32x4 b;
        if (!TRANS) {
            b = *reinterpret_cast<const f32x4*>(W + (size_t)(n0 + i) * M + k0 + 4 * kh);
        } else {
            const float* wp = W + (size_t)(k0 + 4 * kh) * M + n0 + i;
            b.x = wp[0]; b.y = wp[M]; b.z = wp[2 * M]; b.w = wp[3 * M];
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, acc, 0, 0, 0);
    }
}
__device__ __forceinline__ int acc_row(int v) { return (v & 3) + 8 * (v >> 2) + 4 * ((threadIdx.x & 63) >> 5); }
__device__ __forceinline__ int acc_col(int n0) { return n0 + (threadIdx.x & 31); }

// LayerNorm over the rows of a [32][M] LDS image, one wave per 8 rows (in place allowed: a row is read into registers first).
// MODE 0: dst = x_hat;  1: x_hat * g + b;  2: lrelu(x_hat * g + b).  stats (global, may be null): (mean, rstd) of valid rows at
// stats[(row * NS + j) * 2].  mu / rs (LDS, may be null): the row's mean / rstd.
template <int MODE>
__device__ void ln_rows(const float* src, float* dst, int P, int M, const float* __restrict__ g, const float* __restrict__ b,
                        float* stats, int NS, int j, int r0, int B, float* mu, float* rs) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int rr = 0; rr < 8; ++rr) {
        const int r = w * 8 + rr;
        float v[4];
        float s = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = lane + 64 * c;
            v[c] = n < M ? src[r * P + n] : 0.f;
            s += v[c];
        }
        const float mean = wave_sum(s) / (float)M;
        float q = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = lane + 64 * c;
            const float d = v[c] - mean;
            q += n < M ? d * d : 0.f;
        }
        const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)M + LN_EPS);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = lane + 64 * c;
            if (n < M) {
                float o = (v[c] - mean) * rstd;
                if (MODE >= 1) o = o * g[n] + b[n];
                if (MODE == 2) o = lrelu(o);
                dst[r * P + n] = o;
            }
        }
        if (lane == 0) {
            if (mu) { mu[r] = mean; rs[r] = rstd; }
            if (stats && r0 + r < B) { stats[((size_t)(r0 + r) * NS + j) * 2] = mean; stats[((size_t)(r0 + r) * NS + j) * 2 + 1] = rstd; }
        }
    }
}

// LayerNorm backward over rows: dxh = dyn[r][n] * g[n] (dyn: gradient w.r.t. the affine output), x_hat from xh(r, n);
//   out[r][n] (+)= rstd_r * (dxh - mean(dxh) - x_hat * mean(dxh * x_hat))
template <typename XH>
__device__ void ln_bwd_rows(const float* dyn, int P, int M, const float* __restrict__ g, const float* rs, XH xh, float* out, bool add) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int rr = 0; rr < 8; ++rr) {
        const int r = w * 8 + rr;
        float dx[4], xv[4];
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = lane + 64 * c;
            dx[c] = n < M ? dyn[r * P + n] * g[n] : 0.f;
            xv[c] = n < M ? xh(r, n) : 0.f;
            s1 += dx[c];
            s2 += dx[c] * xv[c];
        }
        const float m1 = wave_sum(s1) / (float)M, m2 = wave_sum(s2) / (float)M, rstd = rs[r];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int n = lane + 64 * c;
            if (n < M) {
                const float o = rstd * (dx[c] - m1 - xv[c] * m2);
                out[r * P + n] = add ? out[r * P + n] + o : o;
            }
        }
    }
}

struct FwdArgs {
    const float* x;
    const long long* t;
    ToyW w;
    const float* E;       // [T][M]
    float* y;
    float* saved;         // [L+1][B][M] h_l, then [B][2L+1][2] (mean, rstd); null: inference
    int B, D, M, L, T;
};

__device__ __forceinline__ int row_t(const long long* t, int row, int B, int T) {
    if (row >= B) return 0;
    const long long v = t[row];
    return (v >= 0 && v < T) ? (int)v : -1;                  // -1: outside the table, the row becomes NaN
}

__global__ void __launch_bounds__(NT) toy_fwd_kernel(FwdArgs a) {
    extern __shared__ float sm[];
    const int M = a.M, D = a.D, B = a.B, L = a.L, P = M + 4, NS = 2 * L + 1;
    float* HB = sm;
    float* UB = sm + RT * P;
    float* xs = sm + 2 * RT * P;
    int* ts = reinterpret_cast<int*>(xs + RT * MAXD);
    const int tid = threadIdx.x, w = tid >> 6, r0 = blockIdx.x * RT;
    for (int e = tid; e < RT * D; e += NT) {
        const int r = e / D, d = e - r * D;
        xs[r * MAXD + d] = r0 + r < B ? a.x[(size_t)(r0 + r) * D + d] : 0.f;
    }
    if (tid < RT) ts[tid] = row_t(a.t, r0 + tid, B, a.T);
    __syncthreads();
    for (int e = tid; e < RT * M; e += NT) {                 // in_fc (no bias)
        const int r = e / M, n = e - r * M;
        float s = 0.f;
        for (int d = 0; d < D; ++d) s = fmaf(xs[r * MAXD + d], a.w.win[n * D + d], s);
        HB[r * P + n] = s;
    }
    __syncthreads();
    float* stats = a.saved ? a.saved + (size_t)(L + 1) * B * M : nullptr;
    const int ntiles = M / 32;
    f32x16 acc0, acc1;
    auto put_z = [&](const f32x16& acc, int n0) {
        const int c = acc_col(n0);
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const int r = acc_row(v), tt = ts[r];
            UB[r * P + c] = acc[v] + (tt >= 0 ? a.E[(size_t)tt * M + c] : __builtin_nanf(""));
        }
    };
    for (int l = 0; l < L; ++l) {
        if (a.saved)
            for (int e = tid; e < RT * M; e += NT) {
                const int r = e / M, n = e - r * M;
                if (r0 + r < B) a.saved[((size_t)l * B + r0 + r) * M + n] = HB[r * P + n];
            }
        ln_rows<2>(HB, UB, P, M, a.w.g1, a.w.b1, stats, NS, 2 * l, r0, B, nullptr, nullptr);
        __syncthreads();
        // Z = A1 fc1^T + E[t]: both of a wave's tiles are computed before UB is overwritten
        if (w < ntiles) tile_gemm<false>(UB, P, a.w.fc1, M, 32 * w, acc0);
        if (w + 4 < ntiles) tile_gemm<false>(UB, P, a.w.fc1, M, 32 * (w + 4), acc1);
        __syncthreads();
        if (w < ntiles) put_z(acc0, 32 * w);
        if (w + 4 < ntiles) put_z(acc1, 32 * (w + 4));
        __syncthreads();
        ln_rows<2>(UB, UB, P, M, a.w.g2, a.w.b2, stats, NS, 2 * l + 1, r0, B, nullptr, nullptr);
        __syncthreads();
        for (int n0 = 32 * w; n0 < M; n0 += 128) {
            tile_gemm<false>(UB, P, a.w.fc2, M, n0, acc0);
            const int c = acc_col(n0);
#pragma unroll
            for (int v = 0; v < 16; ++v) HB[acc_row(v) * P + c] += acc0[v];
        }
        __syncthreads();
    }
    if (a.saved)
        for (int e = tid; e < RT * M; e += NT) {
            const int r = e / M, n = e - r * M;
            if (r0 + r < B) a.saved[((size_t)L * B + r0 + r) * M + n] = HB[r * P + n];
        }
    ln_rows<1>(HB, UB, P, M, a.w.gon, a.w.bon, stats, NS, 2 * L, r0, B, nullptr, nullptr);
    __syncthreads();
    for (int e = tid; e < RT * D; e += NT) {                 // out_fc (bias)
        const int r = e / D, d = e - r * D;
        if (r0 + r >= B) continue;
        float s = 0.f;
        for (int n = 0; n < M; ++n) s = fmaf(UB[r * P + n], a.w.wout[d * M + n], s);
        a.y[(size_t)(r0 + r) * D + d] = s + a.w.bout[d];
    }
}

// ---------------------------------------------------------------- backward of the rows
struct BwdArgs {
    const float* x;
    const long long* t;
    const float* dy;
    ToyW w;
    const float* E;
    const float* saved;
    float* dx;            // may be null
    float* opA1;          // [L][B][M]  fc1 input  (A1_l = lrelu(LN1(h_l)))
    float* opDZ;          // [L][B][M]  fc1 output gradient
    float* opG;           // [L][B][M]  fc2 output gradient (dh_{l+1})
    float* opA2;          // [L][B][M]  fc2 input
    float* dzsum;         // [B][M]     sum over layers of dZ_l
    float* tslab;         // [tiles][NP] per-tile partial sums of the small gradients
    int B, D, M, L, T, NP;
};

// small-gradient slab layout per tile: [n1w M][n1b M][n2w M][n2b M][onw M][onb M][win M*D][wout D*M][bout D]
__host__ __device__ inline int small_np(int M, int D) { return 6 * M + 2 * M * D + D; }

__global__ void __launch_bounds__(NT) toy_bwd_kernel(BwdArgs a) {
    extern __shared__ float sm[];
    const int M = a.M, D = a.D, B = a.B, L = a.L, P = M + 4, NS = 2 * L + 1;
    float* HB = sm;
    float* GB = sm + RT * P;
    float* UB = sm + 2 * RT * P;
    float* VB = sm + 3 * RT * P;
    float* xs = sm + 4 * RT * P;
    float* dys = xs + RT * MAXD;
    float* st = dys + RT * MAXD;            // [4][32]: mu1, rs1, mu2, rs2 (the output norm uses mu1 / rs1)
    int* ts = reinterpret_cast<int*>(st + 4 * RT);
    float *mu1 = st, *rs1 = st + RT, *mu2 = st + 2 * RT, *rs2 = st + 3 * RT;
    const int tid = threadIdx.x, w = tid >> 6, r0 = blockIdx.x * RT;
    const float* stats = a.saved + (size_t)(L + 1) * B * M;
    float* slab = a.tslab + (size_t)blockIdx.x * a.NP;
    f32x16 acc;

    for (int e = tid; e < RT * D; e += NT) {
        const int r = e / D, d = e - r * D;
        const bool ok = r0 + r < B;
        xs[r * MAXD + d] = ok ? a.x[(size_t)(r0 + r) * D + d] : 0.f;
        dys[r * MAXD + d] = ok ? a.dy[(size_t)(r0 + r) * D + d] : 0.f;     // rows past B carry no gradient
    }
    if (tid < RT) {
        const bool ok = r0 + tid < B;
        ts[tid] = row_t(a.t, r0 + tid, B, a.T);
        mu1[tid] = ok ? stats[((size_t)(r0 + tid) * NS + 2 * L) * 2] : 0.f;
        rs1[tid] = ok ? stats[((size_t)(r0 + tid) * NS + 2 * L) * 2 + 1] : 1.f;
    }
    __syncthreads();
    // ---- output: x_hat of LN_out in UB, dU = dy W_out in VB
    for (int e = tid; e < RT * M; e += NT) {
        const int r = e / M, n = e - r * M;
        const float h = r0 + r < B ? a.saved[((size_t)L * B + r0 + r) * M + n] : 0.f;
        UB[r * P + n] = (h - mu1[r]) * rs1[r];
        float s = 0.f;
        for (int d = 0; d < D; ++d) s = fmaf(dys[r * MAXD + d], a.w.wout[d * M + n], s);
        VB[r * P + n] = s;
    }
    __syncthreads();
    for (int e = tid; e < D * M; e += NT) {                  // out_fc.weight [D][M]
        const int d = e / M, n = e - d * M;
        const float g = a.w.gon[n], bb = a.w.bon[n];
        float s = 0.f;
        for (int r = 0; r < RT; ++r) s = fmaf(dys[r * MAXD + d], UB[r * P + n] * g + bb, s);
        slab[6 * M + M * D + e] = s;
    }
    if (tid < D) {
        float s = 0.f;
        for (int r = 0; r < RT; ++r) s += dys[r * MAXD + tid];
        slab[6 * M + 2 * M * D + tid] = s;
    }
    if (tid < M) {
        float sg = 0.f, sb = 0.f;
        for (int r = 0; r < RT; ++r) { sg = fmaf(VB[r * P + tid], UB[r * P + tid], sg); sb += VB[r * P + tid]; }
        slab[4 * M + tid] = sg;
        slab[5 * M + tid] = sb;
    }
    ln_bwd_rows(VB, P, M, a.w.gon, rs1, [&](int r, int n) { return UB[r * P + n]; }, GB, false);
    __syncthreads();

    float dg1 = 0.f, db1 = 0.f, dg2 = 0.f, db2 = 0.f;       // column tid's LayerNorm gradients, summed over layers
    for (int l = L - 1; l >= 0; --l) {
        if (tid < RT) {
            const bool ok = r0 + tid < B;
            const size_t s = ((size_t)(r0 + tid) * NS + 2 * l) * 2;
            mu1[tid] = ok ? stats[s] : 0.f;
            rs1[tid] = ok ? stats[s + 1] : 1.f;
            mu2[tid] = ok ? stats[s + 2] : 0.f;
            rs2[tid] = ok ? stats[s + 3] : 1.f;
        }
        __syncthreads();
        for (int e = tid; e < RT * M; e += NT) {
            const int r = e / M, n = e - r * M;
            const bool ok = r0 + r < B;
            const size_t o = ((size_t)l * B + r0 + r) * M + n;
            const float h = ok ? a.saved[o] : 0.f;
            HB[r * P + n] = h;
            const float a1 = lrelu((h - mu1[r]) * rs1[r] * a.w.g1[n] + a.w.b1[n]);
            UB[r * P + n] = a1;
            if (ok) { a.opA1[o] = a1; a.opG[o] = GB[r * P + n]; }
        }
        __syncthreads();
        // Z = A1 fc1^T + E[t] (bit-identical to the forward's), x_hat2 -> VB
        for (int n0 = 32 * w; n0 < M; n0 += 128) {
                tile_gemm<false>(UB, P, a.w.fc1, M, n0, acc);
                const int c = acc_col(n0);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int r = acc_row(v), tt = ts[r];
                    const float z = acc[v] + (tt >= 0 ? a.E[(size_t)tt * M + c] : __builtin_nanf(""));
                    VB[r * P + c] = (z - mu2[r]) * rs2[r];
                }
            }
        __syncthreads();
        for (int e = tid; e < RT * M; e += NT) {
            const int r = e / M, n = e - r * M;
            if (r0 + r < B) a.opA2[((size_t)l * B + r0 + r) * M + n] = lrelu(VB[r * P + n] * a.w.g2[n] + a.w.b2[n]);
        }
        // dP2 = (dh_{l+1} fc2) * lrelu'(P2) -> UB (A1 is no longer read)
        for (int n0 = 32 * w; n0 < M; n0 += 128) {
                tile_gemm<true>(GB, P, a.w.fc2, M, n0, acc);
                const int c = acc_col(n0);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int r = acc_row(v);
                    UB[r * P + c] = lrelu_grad(VB[r * P + c] * a.w.g2[c] + a.w.b2[c], acc[v]);
                }
            }
        __syncthreads();
        if (tid < M) {
            for (int r = 0; r < RT; ++r) { dg2 = fmaf(UB[r * P + tid], VB[r * P + tid], dg2); db2 += UB[r * P + tid]; }
        }
        __syncthreads();
        ln_bwd_rows(UB, P, M, a.w.g2, rs2, [&](int r, int n) { return VB[r * P + n]; }, UB, false);   // dZ (in place, row-owned)
        __syncthreads();
        for (int e = tid; e < RT * M; e += NT) {
            const int r = e / M, n = e - r * M;
            if (r0 + r >= B) continue;
            const float dz = UB[r * P + n];
            a.opDZ[((size_t)l * B + r0 + r) * M + n] = dz;
            float* s = a.dzsum + (size_t)(r0 + r) * M + n;
            *s = l == L - 1 ? dz : *s + dz;
        }
        // dP1 = (dZ fc1) * lrelu'(P1) -> VB
        for (int n0 = 32 * w; n0 < M; n0 += 128) {
                tile_gemm<true>(UB, P, a.w.fc1, M, n0, acc);
                const int c = acc_col(n0);
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int r = acc_row(v);
                    const float xh = (HB[r * P + c] - mu1[r]) * rs1[r];
                    VB[r * P + c] = lrelu_grad(xh * a.w.g1[c] + a.w.b1[c], acc[v]);
                }
            }
        __syncthreads();
        if (tid < M) {
            for (int r = 0; r < RT; ++r) {
                const float xh = (HB[r * P + tid] - mu1[r]) * rs1[r];
                dg1 = fmaf(VB[r * P + tid], xh, dg1);
                db1 += VB[r * P + tid];
            }
        }
        ln_bwd_rows(VB, P, M, a.w.g1, rs1, [&](int r, int n) { return (HB[r * P + n] - mu1[r]) * rs1[r]; }, GB, true);
        __syncthreads();
    }
    if (tid < M) {
        slab[tid] = dg1;
        slab[M + tid] = db1;
        slab[2 * M + tid] = dg2;
        slab[3 * M + tid] = db2;
    }
    for (int e = tid; e < M * D; e += NT) {                  // in_fc.weight [M][D]
        const int n = e / D, d = e - n * D;
        float s = 0.f;
        for (int r = 0; r < RT; ++r) s = fmaf(GB[r * P + n], xs[r * MAXD + d], s);
        slab[6 * M + e] = s;
    }
    if (a.dx)
        for (int e = tid; e < RT * D; e += NT) {
            const int r = e / D, d = e - r * D;
            if (r0 + r >= B) continue;
            float s = 0.f;
            for (int n = 0; n < M; ++n) s = fmaf(GB[r * P + n], a.w.win[n * D + d], s);
            a.dx[(size_t)(r0 + r) * D + d] = s;
        }
}

// decoder gradient buffer: [in_fc.w M*D][norm1.w M][norm1.b M][fc1.w M*M][norm2.w M][norm2.b M][fc2.w M*M][out_norm.w M][out_norm.b M]
//                          [out_fc.w D*M][out_fc.b D]
// one workgroup per element: thread i adds tiles i, i + 256, ... in order, then a fixed-shape tree over the 256 partials (deterministic)
__global__ void __launch_bounds__(256) toy_small_reduce_kernel(const float* __restrict__ tslab, int tiles, int NP, int M, int D,
                                                               float* __restrict__ g) {
    __shared__ float part[256];
    const int e = blockIdx.x, tid = threadIdx.x;
    float s = 0.f;
    for (int i = tid; i < tiles; i += 256) s += tslab[(size_t)i * NP + e];
    part[tid] = s;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    if (tid) return;
    s = part[0];
    const int MD = M * D, MM = M * M;
    int o;
    if (e < 2 * M) o = MD + e;                                   // norm1 w, b
    else if (e < 4 * M) o = MD + 2 * M + MM + (e - 2 * M);       // norm2 w, b
    else if (e < 6 * M) o = MD + 4 * M + 2 * MM + (e - 4 * M);   // out_norm w, b
    else if (e < 6 * M + MD) o = e - 6 * M;                      // in_fc
    else o = MD + 6 * M + 2 * MM + (e - 6 * M - MD);             // out_fc w, b
    g[o] = s;
}

// dW[m][n] = sum_{r < K} P[r][m] Q[r][n] over the rows of split blockIdx.y, one wave per 32 x 32 output tile; z = 0: fc1, 1: fc2
__global__ void __launch_bounds__(64) toy_atb_kernel(const float* P0, const float* Q0, const float* P1, const float* Q1, float* slab,
                                                     int K, int M, int KS, int chunk) {
    const int nt = M / 32, mt = blockIdx.x / nt, ntl = blockIdx.x - mt * nt, s = blockIdx.y, z = blockIdx.z;
    const float* Pm = z ? P1 : P0;
    const float* Qm = z ? Q1 : Q0;
    const int lane = threadIdx.x, i = lane & 31, kh = lane >> 5, m0 = 32 * mt, n0 = 32 * ntl;
    const int kb = s * chunk, ke = min(K, kb + chunk);
    f32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0.f;
    for (int k0 = kb; k0 < ke; k0 += 8) {
        float av[4], bv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int r = k0 + 4 * kh + j;
            av[j] = r < ke ? Pm[(size_t)r * M + m0 + i] : 0.f;
            bv[j] = r < ke ? Qm[(size_t)r * M + n0 + i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[j], bv[j], acc, 0, 0, 0);
    }
    float* out = slab + ((size_t)z * KS + s) * M * M;
#pragma unroll
    for (int v = 0; v < 16; ++v) out[(size_t)(m0 + acc_row(v)) * M + n0 + i] = acc[v];
}

__global__ void toy_atb_reduce_kernel(const float* __restrict__ slab, int KS, int MM, float* g1, float* g2) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y;
    if (e >= MM) return;
    const float* src = slab + (size_t)z * KS * MM + e;
    float s = 0.f, c = 0.f;
    for (int i = 0; i < KS; ++i) {
        const float y = src[(size_t)i * MM] - c, u = s + y;
        c = (u - s) - y;
        s = u;
    }
    (z ? g2 : g1)[e] = s;
}

// ---------------------------------------------------------------- time table
constexpr int TT = 8;    // timesteps per workgroup

__device__ __forceinline__ float temb_value(int tt, int i, int M, const float* freqs) {
    const int half = M / 2;       // same arithmetic as csrc/elementwise.hip temb_kernel (ddpm_timestep_embedding)
    const float arg = __fmul_rn((float)tt, freqs[i < half ? i : i - half]);
    return i < half ? sinf(arg) : cosf(arg);
}

// tabs: E [T][M], then C [T][M] = lrelu(t_proj(temb))
__global__ void __launch_bounds__(NT) toy_tt_fwd_kernel(const float* freqs, const float* tw, const float* tb, const float* ew, const float* eb,
                                                        float* tabs, int T, int M) {
    __shared__ float emb[TT][256];
    __shared__ float cc[TT][256];
    const int t0 = blockIdx.x * TT, tid = threadIdx.x;
    for (int e = tid; e < TT * M; e += NT) {
        const int j = e / M, i = e - j * M;
        emb[j][i] = t0 + j < T ? temb_value(t0 + j, i, M, freqs) : 0.f;
    }
    __syncthreads();
    const int n = tid;
    float s[TT];
    if (n < M) {
#pragma unroll
        for (int j = 0; j < TT; ++j) s[j] = 0.f;
        for (int i = 0; i < M; ++i) {
            const float wv = tw[(size_t)n * M + i];
#pragma unroll
            for (int j = 0; j < TT; ++j) s[j] = fmaf(wv, emb[j][i], s[j]);
        }
#pragma unroll
        for (int j = 0; j < TT; ++j) {
            const float c = lrelu(s[j] + tb[n]);
            cc[j][n] = c;
            if (t0 + j < T) tabs[(size_t)T * M + (size_t)(t0 + j) * M + n] = c;
        }
    }
    __syncthreads();
    if (n < M) {
#pragma unroll
        for (int j = 0; j < TT; ++j) s[j] = 0.f;
        for (int i = 0; i < M; ++i) {
            const float wv = ew[(size_t)n * M + i];
#pragma unroll
            for (int j = 0; j < TT; ++j) s[j] = fmaf(wv, cc[j][i], s[j]);
        }
#pragma unroll
        for (int j = 0; j < TT; ++j)
            if (t0 + j < T) tabs[(size_t)(t0 + j) * M + n] = s[j] + eb[n];
    }
}

// dE[tt][n] = sum, in row order, of dzsum[r][n] over the rows r with t[r] == tt (one workgroup per timestep)
__global__ void __launch_bounds__(NT) toy_tt_gather_kernel(const long long* t, const float* dzsum, float* dE, int B, int M) {
    __shared__ unsigned long long masks[4];
    const int tt = blockIdx.x, tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    float acc = 0.f;
    for (int base = 0; base < B; base += NT) {
        const int r = base + tid;
        const bool hit = r < B && t[r] == (long long)tt;
        const unsigned long long m = __ballot(hit);
        if (lane == 0) masks[w] = m;
        __syncthreads();
        for (int q = 0; q < 4; ++q) {
            unsigned long long mq = masks[q];
            while (mq) {
                const int b = __builtin_ctzll(mq);
                mq &= mq - 1;
                if (tid < M) acc += dzsum[(size_t)(base + 64 * q + b) * M + tid];
            }
        }
        __syncthreads();
    }
    if (tid < M) dE[(size_t)tt * M + tid] = acc;
}

// per timestep: dc = dE enc_w, da = dc * lrelu'(a) (c > 0 <=> a > 0), and the embedding row for the t_proj weight gradient
__global__ void __launch_bounds__(NT) toy_tt_dc_kernel(const float* dE, const float* ew, const float* tabs, const float* freqs,
                                                       float* da, float* emb, int T, int M) {
    __shared__ float row[256];
    const int tt = blockIdx.x, j = threadIdx.x;
    if (j < M) row[j] = dE[(size_t)tt * M + j];
    __syncthreads();
    if (j >= M) return;
    float s = 0.f;
    for (int n = 0; n < M; ++n) s = fmaf(row[n], ew[(size_t)n * M + j], s);
    const float c = tabs[(size_t)T * M + (size_t)tt * M + j];
    da[(size_t)tt * M + j] = c > 0.f ? s : s * SLOPE;
    emb[(size_t)tt * M + j] = temb_value(tt, j, M, freqs);
}

// blocks 0..M-1: enc row n (dW[n][j] = sum_t dE[t][n] c[t][j], db[n] = sum_t dE[t][n]); blocks M..2M-1: t_proj row j (sum_t da[t][j] emb[t][i])
__global__ void __launch_bounds__(NT) toy_tt_wgrad_kernel(const float* dE, const float* da, const float* emb, const float* tabs, float* gt,
                                                          int T, int M) {
    const int b = blockIdx.x, i = threadIdx.x;
    if (i >= M) return;
    const bool enc = b < M;
    const int row = enc ? b : b - M;
    const float* G = enc ? dE : da;
    const float* X = enc ? tabs + (size_t)T * M : emb;
    float s = 0.f, sb = 0.f;
    for (int tt = 0; tt < T; ++tt) {
        const float gv = G[(size_t)tt * M + row];
        s = fmaf(gv, X[(size_t)tt * M + i], s);
        sb += gv;
    }
    const size_t base = enc ? 0 : (size_t)M * M + M;        // gtab: [enc.w][enc.b][t_proj.w][t_proj.b]
    gt[base + (size_t)row * M + i] = s;
    if (i == 0) gt[base + (size_t)M * M + row] = sb;
}

inline bool geom_ok(int D, int M, int L, int T) {
    return D >= 1 && D <= MAXD && M >= 32 && M <= 256 && M % 32 == 0 && L >= 1 && L <= 1024 && T >= 1 && T <= 4096;
}
inline bool fits32(long long floats) { return floats >= 0 && floats * 4 < (1ll << 31); }
inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }
inline long long up64(long long n) { return (n + 63) / 64 * 64; }

int atb_splits(long long K) {
    const long long s = (K + 511) / 512;
    return (int)(s < 1 ? 1 : (s > 64 ? 64 : s));
}

}  // namespace

extern "C" {

int ddpm_toy_time_table(const float* freqs, const float* tproj_w, const float* tproj_b, const float* enc_w, const float* enc_b,
                        float* tabs, int T, int M, void* stream) {
    if (!freqs || !tproj_w || !tproj_b || !enc_w || !enc_b || !tabs) return DDPM_ERR_NULL;
    if (!geom_ok(1, M, 1, T)) return DDPM_ERR_SHAPE;
    hipLaunchKernelGGL(toy_tt_fwd_kernel, dim3(cdiv(T, TT)), dim3(NT), 0, (hipStream_t)stream, freqs, tproj_w, tproj_b, enc_w, enc_b, tabs, T, M);
    return check_launch();
}

int ddpm_toy_decoder_fwd(const float* x, const long long* t, const float* w_in, const float* n1_w, const float* n1_b, const float* fc1_w,
                         const float* n2_w, const float* n2_b, const float* fc2_w, const float* on_w, const float* on_b, const float* out_w,
                         const float* out_b, const float* tabs, float* y, float* saved, int B, int D, int M, int L, int T, void* stream) {
    if (!x || !t || !w_in || !n1_w || !n1_b || !fc1_w || !n2_w || !n2_b || !fc2_w || !on_w || !on_b || !out_w || !out_b || !tabs || !y)
        return DDPM_ERR_NULL;
    if (B < 1 || !geom_ok(D, M, L, T)) return DDPM_ERR_SHAPE;
    if (!fits32((long long)(L + 1) * B * M + (long long)B * (2 * L + 1) * 2) || !fits32((long long)B * D)) return DDPM_ERR_SHAPE;
    if (!aligned16(fc1_w) || !aligned16(fc2_w)) return DDPM_ERR_ALIGN;
    FwdArgs a;
    a.x = x; a.t = t; a.E = tabs; a.y = y; a.saved = saved;
    a.w = ToyW{w_in, n1_w, n1_b, fc1_w, n2_w, n2_b, fc2_w, on_w, on_b, out_w, out_b};
    a.B = B; a.D = D; a.M = M; a.L = L; a.T = T;
    const size_t lds = (size_t)(2 * RT * (M + 4) + RT * MAXD + RT) * 4;
    static DevOnce attr;
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&toy_fwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return DDPM_ERR_LAUNCH;
        attr = true;
    }
    hipLaunchKernelGGL(toy_fwd_kernel, dim3(cdiv(B, RT)), dim3(NT), lds, (hipStream_t)stream, a);
    return check_launch();
}

static long long toy_bwd_ws_floats(int B, int D, int M, int L) {
    const long long K = (long long)L * B;
    return 4 * up64(K * M) + up64((long long)2 * atb_splits(K) * M * M) + up64((long long)cdiv(B, RT) * small_np(M, D));
}

int ddpm_toy_decoder_bwd(const float* x, const long long* t, const float* dy, const float* w_in, const float* n1_w, const float* n1_b,
                         const float* fc1_w, const float* n2_w, const float* n2_b, const float* fc2_w, const float* on_w, const float* on_b,
                         const float* out_w, const float* tabs, const float* saved, float* dx, float* grads, float* dzsum, float* ws,
                         long long ws_floats, int B, int D, int M, int L, int T, void* stream) {
    if (!x || !t || !dy || !w_in || !n1_w || !n1_b || !fc1_w || !n2_w || !n2_b || !fc2_w || !on_w || !on_b || !out_w || !tabs || !saved ||
        !grads || !dzsum || !ws)
        return DDPM_ERR_NULL;
    if (B < 1 || !geom_ok(D, M, L, T)) return DDPM_ERR_SHAPE;
    const long long K = (long long)L * B;
    if (!fits32((L + 1) * (long long)B * M + (long long)B * (2 * L + 1) * 2) || !fits32(K * M) || ws_floats < toy_bwd_ws_floats(B, D, M, L) ||
        !fits32(ws_floats))
        return DDPM_ERR_SHAPE;
    if (!aligned16(fc1_w) || !aligned16(fc2_w)) return DDPM_ERR_ALIGN;
    const int tiles = cdiv(B, RT), KS = atb_splits(K), NP = small_np(M, D);
    BwdArgs a;
    a.x = x; a.t = t; a.dy = dy; a.E = tabs; a.saved = saved; a.dx = dx; a.dzsum = dzsum;
    a.w = ToyW{w_in, n1_w, n1_b, fc1_w, n2_w, n2_b, fc2_w, on_w, on_b, out_w, nullptr};
    a.opA1 = ws; a.opDZ = ws + up64(K * M); a.opG = ws + 2 * up64(K * M); a.opA2 = ws + 3 * up64(K * M);
    float* atb = ws + 4 * up64(K * M);
    a.tslab = atb + up64((long long)2 * KS * M * M);
    a.B = B; a.D = D; a.M = M; a.L = L; a.T = T; a.NP = NP;
    const size_t lds = (size_t)(4 * RT * (M + 4) + 2 * RT * MAXD + 5 * RT) * 4;
    static DevOnce attr;
    if (!attr) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&toy_bwd_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            return DDPM_ERR_LAUNCH;
        attr = true;
    }
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(toy_bwd_kernel, dim3(tiles), dim3(NT), lds, s, a);
    hipLaunchKernelGGL(toy_small_reduce_kernel, dim3(NP), dim3(256), 0, s, a.tslab, tiles, NP, M, D, grads);
    const int chunk = (int)((K + KS - 1) / KS + 7) / 8 * 8;
    hipLaunchKernelGGL(toy_atb_kernel, dim3((M / 32) * (M / 32), KS, 2), dim3(64), 0, s, a.opDZ, a.opA1, a.opG, a.opA2, atb, (int)K, M, KS, chunk);
    const long long MD = (long long)M * D, MM = (long long)M * M;
    hipLaunchKernelGGL(toy_atb_reduce_kernel, dim3(cdiv(MM, 256), 2), dim3(256), 0, s, atb, KS, (int)MM, grads + MD + 2 * M,
                       grads + MD + 4 * M + MM);
    return check_launch();
}

int ddpm_toy_time_table_bwd(const long long* t, const float* dzsum, const float* freqs, const float* enc_w, const float* tabs, float* gtab,
                            float* ws, long long ws_floats, int B, int M, int T, void* stream) {
    if (!t || !dzsum || !freqs || !enc_w || !tabs || !gtab || !ws) return DDPM_ERR_NULL;
    if (B < 1 || !geom_ok(1, M, 1, T)) return DDPM_ERR_SHAPE;
    if (!fits32((long long)B * M) || ws_floats < 3ll * T * M) return DDPM_ERR_SHAPE;
    hipStream_t s = (hipStream_t)stream;
    float *dE = ws, *da = ws + (size_t)T * M, *emb = ws + 2 * (size_t)T * M;
    hipLaunchKernelGGL(toy_tt_gather_kernel, dim3(T), dim3(NT), 0, s, t, dzsum, dE, B, M);
    hipLaunchKernelGGL(toy_tt_dc_kernel, dim3(T), dim3(NT), 0, s, dE, enc_w, tabs, freqs, da, emb, T, M);
    hipLaunchKernelGGL(toy_tt_wgrad_kernel, dim3(2 * M), dim3(NT), 0, s, dE, da, emb, tabs, gtab, T, M);
    return check_launch();
}

}  // extern "C"
