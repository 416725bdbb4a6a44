// Improved precision / recall (upstream metrics/precision_recall.py:43-55,156-164,188-204) without the N x N distance matrix:
// an fp16 MFMA pairwise-distance product whose epilogue keeps, per row, either the smallest distances (k-th-neighbour radii) or one
// "inside some hypersphere" bit (coverage).
//
//   d2(i,j) = max(|r_i|^2 + |c_j|^2 - 2 <r_i, c_j>, 0)     fp32; products of fp16 values accumulated in fp32 on v_mfma_f32_32x32x16_f16
//   d(i,j)  = fp16_rne(sqrtf(d2(i,j)))
//
// One workgroup (4 waves) owns a 128-row tile and one contiguous range of 128-column tiles (the column split).  Every wave
// owns 32 rows x 128 columns of the tile (four 32x32 accumulators), so a row belongs to exactly one wave and its per-row state is never
// shared between waves.  In a 32x32 accumulator the column sits on the lane (lane & 31) and the rows in the 16 registers (register v of
// lane half h is row (v&3) + 8(v>>2) + 4h).
//
// Radii: each row keeps its 16 smallest d2 so far, sorted, in LDS, and every lane carries the current rank-th smallest of its 16 rows in
// registers.  A new value is compared against that threshold; the few that pass (about rank * ln(columns / rank) per row once the list has
// warmed up) are inserted one at a time by the owning wave.  sqrt and the fp16 rounding are monotone, so the selection runs on d2.  The
// lists of the column splits go to the workspace and a second kernel picks the rank-th smallest of their union: a multiset operation,
// independent of the order anything arrived in — bit-deterministic without atomics.
//
// Coverage: the epilogue rounds d to fp16 and compares it with the fp16 radius of its column; a lane collects one bit per row register
// and the wave stores a 1 into hit[row] at the end (plain byte stores of the same value into an array the pre-pass zeroed).
//
// The pre-pass writes the fp32 squared norms of both operands into the workspace.  Nothing allocates or synchronises.
#include "common.h"

#include <hip/hip_fp16.h>

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

constexpr int TM = 128;             // rows per workgroup
constexpr int TN = 128;             // columns per step
constexpr int BK = 64;              // reduction elements per LDS stage
constexpr int LDP = BK + 8;         // LDS row pitch in halves (144 B: 16-byte aligned, rows spread over the banks)
constexpr int NT = 256;
constexpr int VPR = BK / 8;         // 16-byte vectors per staged row
constexpr int RPP = NT / VPR;       // rows one pass of the workgroup stages
constexpr int LDV = TM / RPP;       // vectors per thread, operand and stage
constexpr int CAND = 16;            // candidates kept per row = the largest served rank
constexpr int MAX_SPLITS = 64;
constexpr int TARGET_BLOCKS = 4096;  // several rounds of the chip's 512 resident workgroups: the last, partly filled round costs little
constexpr int RESIDENT = 512;

__device__ __forceinline__ float clamp0(float x) { return x < 0.f ? 0.f : x; }      // keeps NaN, like torch's clamp_min

static inline int cdiv(long long a, long long b) { return (int)((a + b - 1) / b); }

// the column split of a geometry (documented in include/ddpm_hip.h: the workspace size depends on it)
static inline void split_of(int Nr, int Nc, int* splits, int* tiles_per_split) {
    const int rt = cdiv(Nr, TM), ct = cdiv(Nc, TN);
    int s0 = cdiv(TARGET_BLOCKS, rt);
    if (s0 > MAX_SPLITS) s0 = MAX_SPLITS;
    if (s0 > ct) s0 = ct;
    const int half = cdiv(ct, 2);                          // two or more steps per split (the first fills the candidate lists) once that
    if ((long long)rt * half >= RESIDENT && s0 > half) s0 = half;      // still fills the chip
    const int tps = cdiv(ct, s0);
    *tiles_per_split = tps;
    *splits = cdiv(ct, tps);
}

// |x|^2 of every row of both operands in fp32 (one wave per row, fixed order); MODE 1 also zeroes hit[0 .. Nr)
__global__ __launch_bounds__(NT) void manifold_norms_kernel(const _Float16* __restrict__ R, unsigned r_ld, int Nr, const _Float16* __restrict__ C,
                                                            unsigned c_ld, int Nc, int D, float* __restrict__ rn, float* __restrict__ cn,
                                                            unsigned char* __restrict__ hit) {
    const int gid = blockIdx.x * NT + threadIdx.x;
    if (hit && gid < Nr) hit[gid] = 0;
    const int row = gid >> 6, lane = threadIdx.x & 63;
    if (row >= Nr + Nc) return;
    const _Float16* src = row < Nr ? R + (size_t)row * r_ld : C + (size_t)(row - Nr) * c_ld;
    float s = 0.f;
    for (int k = lane * 8; k < D; k += 64 * 8) {
        const h16x8 v = *reinterpret_cast<const h16x8*>(src + k);
#pragma unroll
        for (int j = 0; j < 8; ++j) { const float f = (float)v[j]; s = fmaf(f, f, s); }
    }
    s = wave_sum(s);
    if (lane == 0) (row < Nr ? rn[row] : cn[row - Nr]) = s;
}

template <int MODE>      // 0: radii (candidate lists), 1: coverage bits
__global__ __launch_bounds__(NT) void manifold_tile_kernel(const _Float16* __restrict__ R, unsigned r_ld, int Nr, const _Float16* __restrict__ C,
                                                           unsigned c_ld, int Nc, int D, int rank, int splits, int tiles_per_split, int col_tiles,
                                                           const float* __restrict__ rn_g, const float* __restrict__ cn_g,
                                                           float* __restrict__ cand_g, const _Float16* __restrict__ kth,
                                                           unsigned char* __restrict__ hit) {
    __shared__ __attribute__((aligned(16))) _Float16 sA[TM * LDP];
    __shared__ __attribute__((aligned(16))) _Float16 sB[TN * LDP];
    __shared__ float sCand[MODE == 0 ? TM * CAND : 4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    // Consecutive workgroup ids go round-robin to the 8 XCDs, each with its own L2.  Id w -> XCD x = w & 7, q = w >> 3 counts on that XCD:
    // the ~64 workgroups resident there are `splits` column ranges of a few row tiles, so a row tile's stages are fetched by `splits`
    // workgroups and a column step's by several row tiles out of the same L2 (a row tile alone is D * 256 bytes: 1 MB at D = 4096).
    const int q = blockIdx.x >> 3;
    const int split = q % splits;
    const int row_tile = (q / splits) * 8 + (blockIdx.x & 7);
    if (row_tile * TM >= Nr) return;                           // the padding of the row tiles to a multiple of 8 (whole workgroup, before any barrier)
    const int r0 = row_tile * TM;
    const int t0 = split * tiles_per_split;
    const int t1 = t0 + tiles_per_split < col_tiles ? t0 + tiles_per_split : col_tiles;
    const float INF = __builtin_inff();

    float rn[16], thr[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) {
        const int row = r0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
        rn[v] = row < Nr ? rn_g[row] : 0.f;
        thr[v] = INF;
    }
    unsigned hitmask = 0;
    if (MODE == 0) {
#pragma unroll
        for (int i = 0; i < 8; ++i) sCand[(wave * 32 + i * 4 + (lane >> 4)) * CAND + (lane & 15)] = INF;   // this wave's own 32 rows
    }

    const int nk = (D + BK - 1) / BK;
    // global -> register staging: 128 rows x BK / 8 vectors of 16 B per operand and stage, LDV + LDV per thread
    const int ld_row = tid / VPR, ld_k = (tid % VPR) * 8;

    for (int t = t0; t < t1; ++t) {
        const int c0 = t * TN;
        f32x16 acc[4];
#pragma unroll
        for (int ni = 0; ni < 4; ++ni)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[ni][v] = 0.f;

        u32x4 pa[LDV], pb[LDV];
        auto fetch = [&](int kc) {
            const int k = kc * BK + ld_k;
#pragma unroll
            for (int i = 0; i < LDV; ++i) {
                const int gr = r0 + ld_row + RPP * i, gc = c0 + ld_row + RPP * i;
                pa[i] = (gr < Nr && k < D) ? ldg16(R + (size_t)gr * r_ld + k) : zero16();
                pb[i] = (gc < Nc && k < D) ? ldg16(C + (size_t)gc * c_ld + k) : zero16();
            }
        };
        fetch(0);
        for (int kc = 0; kc < nk; ++kc) {
            __syncthreads();                                   // the previous stage has been consumed
#pragma unroll
            for (int i = 0; i < LDV; ++i) {
                *reinterpret_cast<u32x4*>(&sA[(ld_row + RPP * i) * LDP + ld_k]) = pa[i];
                *reinterpret_cast<u32x4*>(&sB[(ld_row + RPP * i) * LDP + ld_k]) = pb[i];
            }
            __syncthreads();
            if (kc + 1 < nk) fetch(kc + 1);                    // in flight under the MFMAs below
#pragma unroll
            for (int kk = 0; kk < BK / 16; ++kk) {
                const h16x8 a = *reinterpret_cast<const h16x8*>(&sA[(wave * 32 + lr) * LDP + kk * 16 + lh * 8]);
#pragma unroll
                for (int ni = 0; ni < 4; ++ni) {
                    const h16x8 b = *reinterpret_cast<const h16x8*>(&sB[(ni * 32 + lr) * LDP + kk * 16 + lh * 8]);
                    acc[ni] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, acc[ni], 0, 0, 0);
                }
            }
        }

        // ---- epilogue of this 128 x 128 step: lane (lr, lh) holds column c0 + 32 ni + lr of rows (v&3) + 8(v>>2) + 4 lh
        if (MODE == 0) {
            float cn[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) { const int c = c0 + ni * 32 + lr; cn[ni] = c < Nc ? cn_g[c] : INF; }   // absent column: never a candidate
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    float d2 = clamp0(rn[v] + cn[ni] - 2.f * acc[ni][v]);
                    for (;;) {
                        const unsigned long long m = __ballot(d2 < thr[v]);
                        if (!m) break;
                        // insert the value of the first such lane into its row's sorted list (lanes 0..15 move one slot each)
                        const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)m) - 1);
                        const float x = __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)__float_as_uint(d2), l));
                        const int h = l >> 5;
                        volatile float* list = sCand + (wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * h) * CAND;
                        const int j = lane & 15;
                        const float c = list[j];
                        const float p = j ? list[j - 1] : -INF;
                        const float nc = c <= x ? c : (p <= x ? x : p);
                        __builtin_amdgcn_wave_barrier();
                        if (lane < 16) list[j] = nc;
                        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        const float nthr = list[rank - 1];
                        if (lh == h) thr[v] = nthr;
                        if (lane == l) d2 = INF;
                    }
                }
            }
        } else {
            float cn[4], kf[4];
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
                const int c = c0 + ni * 32 + lr;
                cn[ni] = c < Nc ? cn_g[c] : 0.f;
                kf[ni] = c < Nc ? (float)kth[c] : -1.f;            // absent column: no distance is <= -1
            }
#pragma unroll
            for (int ni = 0; ni < 4; ++ni) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const float d2 = clamp0(rn[v] + cn[ni] - 2.f * acc[ni][v]);
                    const float d = (float)(_Float16)sqrtf(d2);   // fp16 round-to-nearest-even, overflow -> inf; compared as fp16 values
                    hitmask |= (d <= kf[ni] ? 1u : 0u) << v;
                }
            }
        }
    }

    if (MODE == 0) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int row = wave * 32 + i * 4 + (lane >> 4);
            if (r0 + row < Nr) cand_g[((size_t)split * Nr + r0 + row) * CAND + (lane & 15)] = sCand[row * CAND + (lane & 15)];
        }
    } else {
#pragma unroll
        for (int v = 0; v < 16; ++v) {
            const unsigned long long m = __ballot((hitmask >> v) & 1u);
            const unsigned mine = lh ? (unsigned)(m >> 32) : (unsigned)m;
            const int row = r0 + wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * lh;
            if (lr == 0 && mine && row < Nr) hit[row] = 1;
        }
    }
}

// out[i] = fp16(sqrt(rank-th smallest of the union of the splits' lists)), equal values counted with multiplicity: walk the distinct
// values upwards, counting, until `rank` elements are covered (no per-thread array, nothing that depends on arrival order)
__global__ __launch_bounds__(NT) void manifold_kth_merge_kernel(const float* __restrict__ cand, int Nr, int splits, int rank, _Float16* __restrict__ out) {
    const int i = blockIdx.x * NT + threadIdx.x;
    if (i >= Nr) return;
    float prev = -__builtin_inff(), cur = 0.f;
    int covered = 0;
    while (covered < rank) {
        cur = __builtin_inff();
        int cnt = 0;
        for (int s = 0; s < splits; ++s) {
            const float* list = cand + ((size_t)s * Nr + i) * CAND;
            for (int j = 0; j < rank; ++j) {
                const float x = list[j];
                if (x > prev) {
                    if (x < cur) { cur = x; cnt = 1; }
                    else if (x == cur) ++cnt;
                }
            }
        }
        if (cnt == 0) break;            // fewer than rank finite entries (NaN inputs): report the largest seen
        covered += cnt;
        prev = cur;
    }
    out[i] = (_Float16)sqrtf(cur);
}

int check_operands(const void* r, long long r_ld, int Nr, const void* c, long long c_ld, int Nc, int D) {
    if (Nr < 1 || Nc < 1 || D < 8 || D % 8 != 0 || r_ld < D || c_ld < D) return DDPM_ERR_SHAPE;
    if ((long long)Nr * r_ld * 2 >= (1ll << 31) || (long long)Nc * c_ld * 2 >= (1ll << 31)) return DDPM_ERR_SHAPE;
    return DDPM_OK;
}

int check_alignment(const void* r, long long r_ld, const void* c, long long c_ld, const void* ws) {
    return (aligned16(r) && aligned16(c) && aligned16(ws) && r_ld % 8 == 0 && c_ld % 8 == 0) ? DDPM_OK : DDPM_ERR_ALIGN;
}

}  // namespace

extern "C" {

int ddpm_manifold_kth_f16(const void* rows, long long rows_ld, int Nr, const void* cols, long long cols_ld, int Nc, int D, int rank,
                          void* out, void* workspace, long long workspace_bytes, void* stream) {
    if (!rows || !cols || !out || !workspace) return DDPM_ERR_NULL;
    if (int rc = check_operands(rows, rows_ld, Nr, cols, cols_ld, Nc, D)) return rc;
    if (rank < 1 || rank > CAND || rank > Nc) return DDPM_ERR_SHAPE;
    int splits, tps;
    split_of(Nr, Nc, &splits, &tps);
    const long long need = 4ll * ((long long)Nr + Nc) + 4ll * CAND * splits * (long long)Nr;
    if (workspace_bytes < need) return DDPM_ERR_SHAPE;
    if (int rc = check_alignment(rows, rows_ld, cols, cols_ld, workspace)) return rc;
    float* cand = (float*)workspace;                       // [splits][Nr][16], 16-byte aligned rows
    float* rn = cand + (size_t)CAND * splits * Nr;
    float* cn = rn + Nr;
    const _Float16 *R = (const _Float16*)rows, *C = (const _Float16*)cols;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(manifold_norms_kernel, dim3(cdiv(((long long)Nr + Nc) * 64, NT)), dim3(NT), 0, st, R, (unsigned)rows_ld, Nr, C,
                       (unsigned)cols_ld, Nc, D, rn, cn, (unsigned char*)nullptr);
    hipLaunchKernelGGL(manifold_tile_kernel<0>, dim3(cdiv(cdiv(Nr, TM), 8) * 8 * splits), dim3(NT), 0, st, R, (unsigned)rows_ld, Nr, C, (unsigned)cols_ld, Nc, D,
                       rank, splits, tps, cdiv(Nc, TN), (const float*)rn, (const float*)cn, cand, (const _Float16*)nullptr, (unsigned char*)nullptr);
    hipLaunchKernelGGL(manifold_kth_merge_kernel, dim3(cdiv(Nr, NT)), dim3(NT), 0, st, (const float*)cand, Nr, splits, rank, (_Float16*)out);
    return check_launch();
}

int ddpm_manifold_cover_f16(const void* probe, long long probe_ld, int Np, const void* support, long long support_ld, int Ns, int D,
                            const void* support_kth, void* hit, void* workspace, long long workspace_bytes, void* stream) {
    if (!probe || !support || !support_kth || !hit || !workspace) return DDPM_ERR_NULL;
    if (int rc = check_operands(probe, probe_ld, Np, support, support_ld, Ns, D)) return rc;
    if (workspace_bytes < 4ll * ((long long)Np + Ns)) return DDPM_ERR_SHAPE;
    if (int rc = check_alignment(probe, probe_ld, support, support_ld, workspace)) return rc;
    int splits, tps;
    split_of(Np, Ns, &splits, &tps);
    float* rn = (float*)workspace;
    float* cn = rn + Np;
    const _Float16 *R = (const _Float16*)probe, *C = (const _Float16*)support;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(manifold_norms_kernel, dim3(cdiv(((long long)Np + Ns) * 64, NT)), dim3(NT), 0, st, R, (unsigned)probe_ld, Np, C,
                       (unsigned)support_ld, Ns, D, rn, cn, (unsigned char*)hit);
    hipLaunchKernelGGL(manifold_tile_kernel<1>, dim3(cdiv(cdiv(Np, TM), 8) * 8 * splits), dim3(NT), 0, st, R, (unsigned)probe_ld, Np, C, (unsigned)support_ld, Ns,
                       D, 1, splits, tps, cdiv(Ns, TN), (const float*)rn, (const float*)cn, (float*)nullptr, (const _Float16*)support_kth, (unsigned char*)hit);
    return check_launch();
}

}  // extern "C"
