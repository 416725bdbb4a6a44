// Attention of AttentionBlock (ddpm_torch/models/unet.py:41-52 of tqch/ddpm-torch) at ANY token count and any head count: streaming
// flash forward and backward (gfx950, bf16 operands, fp32 accumulation).  attention.hip keeps one 128 x L score block on chip and
// therefore stops at 256 tokens; here the other side of the score matrix is streamed through LDS in tiles of BN tokens and the
// softmax is the online one, so no L x L object exists anywhere and no L appears as a memory row.  The reference's block is the
// single head (C = the block's channels); with heads > 1 (ADM's QKVAttention ordering) a problem is one (image, head) pair and C
// below is the head's width — see StreamArgs.
//
//     S = Q K^T / sqrt(C)      P = softmax_keys(S)      O = P V                                  (forward)
//     dV = P^T dO      dP = dO V^T      dS = P o (dP - D),  D = rowsum(dO o O)      dQ = dS K / sqrt(C)      dK = dS^T Q / sqrt(C)
//
// One shape for the three kernels.  A workgroup (4 waves) OWNS a block of rows — queries in the forward and in dQ, keys in dK / dV —
// and each wave owns 16 MT of them outright: their operand fragments stay in registers for the kernel's life, and nothing is ever
// exchanged between waves except the streamed tiles.  All products are v_mfma_f32_16x16x32_bf16 in the TRANSPOSED sense
//   score tile   T[streamed 16][own 16]  = Y_tile . X_own^T     A = the streamed rows (ds_read_b128 from LDS), B = the own fragment:
//                lane (ln = lane & 15, g = lane >> 4) then holds own row ln and the four streamed rows 4 g .. 4 g + 3 of a 16-tile, so
//                every per-own-row quantity (running max, running sum, lse, D) is ONE register per lane, a reduction over the streamed
//                side is in-lane plus two shuffles (xor 16, 32), and the bf16 tile goes to LDS as 8-byte writes [own row][streamed];
//   output tile  Z^T[channel 16][own 16] = Y_tile^T . tile^T    A = the streamed operand as stored, pixel-major, read with the hardware
//                transpose (ds_read_b64_tr_b16), B = the bf16 tile (ds_read_b128 of the wave's own LDS region): the accumulators hold four
//                consecutive channels of own row ln — the online rescale is a per-lane scalar and the final store is 8 bytes.
// The streamed side moves as UNITS of [BN tokens][<= 256 channels] (<= 16 KiB) through a three-slot LDS-DMA ring with counted waits,
// two units ahead, one barrier per unit; C > 256 is two units per operand.  A unit is staged once per USE: a tile that is read both
// channel-contiguous (score product) and transposed (output product) is requested twice, each time with the chunk swizzle of its read
// pattern (the second request hits in L2).  Tokens past L are requested out of the descriptor's range: the DMA writes zeros, and
// the element-wise step gives them probability 0 by index, never through exp.  Static LDS <= 64 KiB: no attribute call, nothing
// that a stream capture would see.
#include "common.h"
#include "attention_common.h"
#include <string.h>

namespace {

constexpr int NT = 256;                         // 4 waves
constexpr float NEG_BIG = -3.0e38f;             // "no key seen yet": finite, so the first rescale is exp(-huge) = 0, never exp(-inf + inf)

// 8-byte LDS write next to an LDS-DMA in flight (asm for the reason lds_rd16 is: hipcc would drain the ring in front of it)
__device__ __forceinline__ void lds_wr8(unsigned addr, unsigned lo, unsigned hi) {
    uint2 v; v.x = lo; v.y = hi;
    asm volatile("ds_write_b64 %0, %1" :: "v"(addr), "v"(v) : "memory");
}
__device__ __forceinline__ void vm_wait_units(int n) {
    switch (n) {
    case 0: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
    case 1: asm volatile("s_waitcnt vmcnt(1)" ::: "memory"); break;
    case 2: asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); break;
    case 3: asm volatile("s_waitcnt vmcnt(3)" ::: "memory"); break;
    default: asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); break;
    }
}

// One problem = one (image b, head h): blockIdx.y = b * heads + h.  The kernels see C = the HEAD's width d; the thirds of the packed
// buffer are heads * C apart, and head h of every operand and output is channels [h C, (h + 1) C) of its third — a base offset of
// h C elements and a descriptor that spans C channels from there, so the ring's `ch < C` zero-fill and every bound below are per head.
struct StreamArgs {
    const bf16_t *q, *k, *v;  long long qkv_ld;   // packed projection buffer: q at +0, k at +heads C, v at +2 heads C (pointers already offset)
    const bf16_t *o, *d_o;    long long o_ld, do_ld;
    bf16_t *out;              long long out_ld;    // forward: O
    bf16_t *dq, *dk, *dv;     long long dqkv_ld;
    float *lse, *dvec;                             // [B][heads][L] fp32: row log-sum-exp of the scaled logits; D = rowsum(dO o O)
    int B, L, C, heads;
    float scale;
};

// compile-time geometry of a channel bucket CB (C <= CB)
template <int CB> struct Geo {
    static constexpr int BN = CB <= 128 ? 64 : 32;          // streamed tokens per tile
    static constexpr int NJ = BN / 16;                      // 16-token tiles of it
    static constexpr int CH = CB < 256 ? CB : 256;          // channels of a unit
    static constexpr int NHM = CB > 256 ? 2 : 1;            // units per operand tile
    static constexpr int KSH = CH / 32, NCTH = CH / 16;     // k-steps / 16-channel tiles per unit
    static constexpr int KST = CB / 32, NCTT = CB / 16;     // ... per operand
    static constexpr int SLOTB = BN * CH * 2;               // ring slot (<= 16 KiB)
    static constexpr int PM = BN / 8 - 1;                   // chunk swizzle mask of the bf16 tile's rows
};

// run-time geometry (wave-uniform)
struct Rt {
    int L, C, nch, rowb, swm, nh, per;
};
__device__ __forceinline__ Rt make_rt(int L, int C, int BN) {
    Rt r;
    r.L = L; r.C = C;
    const int cu = C < 256 ? C : 256;
    r.nch = cu >> 3;                                        // 16-byte chunks per staged row: a multiple of 4
    r.rowb = cu * 2;
    int span = 4;
    while (span < 16 && r.nch % (span * 2) == 0) span *= 2; // the XOR must map a row's chunks onto themselves
    r.swm = span - 1;
    r.nh = C > 256 ? 2 : 1;
    r.per = (BN * r.nch + NT - 1) / NT;                     // DMA instructions per thread and unit (<= 4)
    return r;
}
// chunk swizzle of a staged row.  tk = 0, channel-contiguous reads (16 rows at one logical chunk per ds_read_b128 group): the row's
// low bits.  tk = 1, transpose reads (a 16-lane group touches 4 rows x 32 bytes, the half wave rows r .. r+3 and r+8 .. r+11): bits 1-3,
// so that a row's two adjacent chunks stay adjacent and the eight rows land on eight different chunk pairs.
__device__ __forceinline__ int swz(int row, int tk, int swm) {
    const int f = tk ? (((row & 3) << 1) | (((row >> 3) & 1) << 3)) : (row & 15);
    return f & swm;
}

template <int CB>
struct Ring {
    int prow[4], ppc[4];
    int wave;
    char* base;
    __device__ __forceinline__ void init(char* smem, int tid, const Rt& rt) {
        base = smem;
        wave = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int p = i * NT + tid;
            prow[i] = p / rt.nch;
            ppc[i] = p - prow[i] * rt.nch;
        }
    }
    // unit = rows row0 .. row0 + BN of Y, channels 256 h .. of it, into ring slot `slot`; rows >= L and channels >= C: zeros
    __device__ __forceinline__ void issue(const Opnd& Y, int row0, int h, int tk, int slot, const Rt& rt) const {
        char* dst = base + slot * Geo<CB>::SLOTB;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < rt.per) {
                const int row = prow[i], lc = ppc[i] ^ swz(row, tk, rt.swm), ch = h * 256 + lc * 8;
                const bool ok = row < Geo<CB>::BN && row0 + row < rt.L && ch < rt.C;
                unsigned o = ok ? (unsigned)(((long long)(row0 + row) * Y.ld + ch) * 2) : BUF_OOB;
                asm volatile("" : "+v"(o));
                LDS_DMA16(Y.rsrc, dst + (i * NT + wave * 64) * 16, o, 0);
            }
        }
    }
};

// own fragments: rows wr0 + 16 mt + ln of X, k-step ks = channels 32 ks + 8 g .. + 7 (rows >= L: zeros)
template <int CB, int MT>
__device__ __forceinline__ void load_own(u32x4 (&f)[MT][Geo<CB>::KST], const Opnd& X, int wr0, int L, int C, int ln, int g) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int ks = 0; ks < Geo<CB>::KST; ++ks) {
            const int row = wr0 + mt * 16 + ln;
            if (ks * 32 < C) f[mt][ks] = ldv(X, row < L ? (unsigned)(((long long)row * X.ld + ks * 32 + g * 8) * 2) : BUF_OOB);
            else f[mt][ks] = zero16();
        }
}

// score product over one unit (half H of the channels): acc[mt][j] (streamed 16-tile j x own 16-tile mt) += Y_unit . X_own^T
template <int CB, int MT, int H>
__device__ __forceinline__ void prod_s(f32x4 (&acc)[MT][Geo<CB>::NJ], const u32x4 (&own)[MT][Geo<CB>::KST], unsigned cur, int nks, const Rt& rt,
                                       int ln, int g) {
    using G = Geo<CB>;
    unsigned rb[G::NJ];
#pragma unroll
    for (int j = 0; j < G::NJ; ++j) rb[j] = cur + (unsigned)((j * 16 + ln) * rt.rowb);
    const int x = swz(ln, 0, rt.swm);
    u32x4 f[2][G::NJ];
    auto rd = [&](int ks, int set) {
        const unsigned co = (unsigned)(((ks * 4 + g) ^ x) << 4);
#pragma unroll
        for (int j = 0; j < G::NJ; ++j) f[set][j] = lds_rd16(rb[j] + co);
    };
    rd(0, 0);
#pragma unroll
    for (int ks = 0; ks < G::KSH; ++ks) {
        if (ks < nks) {
            if (ks + 1 < nks) { rd(ks + 1, (ks + 1) & 1); lds_wait_n<G::NJ>(); } else lds_wait();
#pragma unroll
            for (int j = 0; j < G::NJ; ++j)
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    acc[mt][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(f[ks & 1][j]), as_frag(own[mt][H * G::KSH + ks]), acc[mt][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
}

// output product over one unit: acc[mt][CT0 + ct] (channel 16-tile ct of the unit x own 16-tile mt) += Y_unit^T . tile^T, the bf16
// tile [16 MT own rows][BN streamed] at LDS address pa
template <int CB, int MT, int NACC, int CT0>
__device__ __forceinline__ void prod_t(f32x4 (&acc)[MT][NACC], unsigned cur, unsigned pa, int nct, const Rt& rt, int ln, int g) {
    using G = Geo<CB>;
#pragma unroll
    for (int kk = 0; kk < G::BN / 32; ++kk) {
        u32x4 fb[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
            fb[mt] = lds_rd16(pa + (unsigned)((mt * 16 + ln) * (G::BN * 2) + (((kk * 4 + g) ^ (ln & G::PM)) << 4)));
        const int krow = kk * 32 + g * 8 + (ln >> 2), xs = swz(krow, 1, rt.swm), lcl = (ln & 3) >> 1;
        const unsigned rbase = cur + (unsigned)(krow * rt.rowb + (ln & 1) * 8);
        uint2 v[2][2];
        auto rd = [&](int ct, int set) {
            const unsigned a0 = rbase + (unsigned)(((ct * 2 + lcl) ^ xs) << 4);
            v[set][0] = lds_rd_tr(a0);
            v[set][1] = lds_rd_tr(a0 + (unsigned)(4 * rt.rowb));           // rows + 4: the same swizzle key
        };
        rd(0, 0);
#pragma unroll
        for (int ct = 0; ct < G::NCTH; ++ct) {
            if (ct < nct) {
                if (ct + 1 < nct) { rd(ct + 1, (ct + 1) & 1); lds_wait_n<2>(); } else lds_wait();
                u32x4 a4; a4.x = v[ct & 1][0].x; a4.y = v[ct & 1][0].y; a4.z = v[ct & 1][1].x; a4.w = v[ct & 1][1].y;
#pragma unroll
                for (int mt = 0; mt < MT; ++mt)
                    acc[mt][CT0 + ct] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(as_frag(a4), as_frag(fb[mt]), acc[mt][CT0 + ct], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
}

// the wave's bf16 tile: values of streamed tokens 16 j + 4 g .. + 3 for own row 16 mt + ln -> [own row][streamed], 8 bytes per write
template <int CB, int MT, typename F>
__device__ __forceinline__ void write_tile(unsigned pa, int ln, int g, F&& f) {
    using G = Geo<CB>;
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int j = 0; j < G::NJ; ++j) {
            const unsigned ad = pa + (unsigned)((mt * 16 + ln) * (G::BN * 2) + (((j * 2 + (g >> 1)) ^ (ln & G::PM)) << 4) + (g & 1) * 8);
            lds_wr8(ad, pack_bf2(f(mt, j, 0), f(mt, j, 1)), pack_bf2(f(mt, j, 2), f(mt, j, 3)));
        }
}

// Z^T accumulators -> out rows wr0 + 16 mt + ln, channels c0 + 16 ct + 4 g .. + 3 (8-byte stores; rows >= L are never stored)
template <int MT, int NACC>
__device__ __forceinline__ void store_own(const f32x4 (&z)[MT][NACC], bf16_t* out, long long ld, int wr0, int L, int c0, int cend, int ln, int g) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int row = wr0 + mt * 16 + ln;
        if (row >= L) continue;
        bf16_t* p = out + (long long)row * ld + c0 + g * 4;
#pragma unroll
        for (int ct = 0; ct < NACC; ++ct) {
            if (c0 + ct * 16 >= cend) continue;
            uint2 w; w.x = pack_bf2(z[mt][ct][0], z[mt][ct][1]); w.y = pack_bf2(z[mt][ct][2], z[mt][ct][3]);
            *reinterpret_cast<uint2*>(p + ct * 16) = w;
        }
    }
}

template <int CB, int MT> struct Smem { static constexpr int PB = 16 * MT * Geo<CB>::BN * 2, BYTES = 3 * Geo<CB>::SLOTB + 4 * PB; };

// the ring's step: wait for unit u (this thread's part, then everyone's), request unit u + 2 into the slot everyone has left
#define STREAM_STEP_BEGIN()                                                    \
    vm_wait_units(u + 1 < nunits ? rt.per : 0);                                \
    __builtin_amdgcn_s_barrier();                                              \
    if (u + 2 < nunits) issue_unit(u + 2, sl == 0 ? 2 : sl - 1);               \
    const unsigned cur = ring0 + (unsigned)(sl * G::SLOTB);                    \
    ++u; sl = sl == 2 ? 0 : sl + 1

// ------------------------------------------------------------------------------------------------ forward
template <int CB, int MT>
__global__ __launch_bounds__(NT)
void attn_stream_fwd_kernel(StreamArgs a) {
    using G = Geo<CB>;
    __shared__ __attribute__((aligned(16))) char smem[Smem<CB, MT>::BYTES];
    const int tid = threadIdx.x, lane = tid & 63, ln = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bh = blockIdx.y, b = bh / a.heads, hc = (bh - b * a.heads) * a.C, wr0 = blockIdx.x * (64 * MT) + wave * (16 * MT);
    const Rt rt = make_rt(a.L, a.C, G::BN);
    const Opnd Q = make_opnd(a.q + (long long)b * a.L * a.qkv_ld + hc, a.qkv_ld, a.L, a.C);
    const Opnd K = make_opnd(a.k + (long long)b * a.L * a.qkv_ld + hc, a.qkv_ld, a.L, a.C);
    const Opnd V = make_opnd(a.v + (long long)b * a.L * a.qkv_ld + hc, a.qkv_ld, a.L, a.C);
    u32x4 qf[MT][G::KST];
    load_own<CB, MT>(qf, Q, wr0, a.L, a.C, ln, g);
    Ring<CB> ring;
    ring.init(smem, tid, rt);
    const unsigned ring0 = lds_addr(smem), pa = ring0 + (unsigned)(3 * G::SLOTB + wave * Smem<CB, MT>::PB);
    const int upt = 2 * rt.nh, nunits = ((a.L + G::BN - 1) / G::BN) * upt;
    auto issue_unit = [&](int uu, int slot) {
        const int t = uu / upt, w = uu - t * upt;
        if (w < rt.nh) ring.issue(K, t * G::BN, w, 0, slot, rt);
        else ring.issue(V, t * G::BN, w - rt.nh, 1, slot, rt);
    };
    issue_unit(0, 0);
    issue_unit(1, 1);                                             // (nunits >= 2)
    f32x4 o[MT][G::NCTT];
    float m[MT], lsum[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        m[mt] = NEG_BIG; lsum[mt] = 0.f;
#pragma unroll
        for (int ct = 0; ct < G::NCTT; ++ct) o[mt][ct] = (f32x4)(0.f);
    }
    int u = 0, sl = 0;
    for (int k0 = 0; k0 < a.L; k0 += G::BN) {
        f32x4 s[MT][G::NJ];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < G::NJ; ++j) s[mt][j] = (f32x4)(0.f);
        static_for<G::NHM>([&](auto hc) {
            constexpr int H = decltype(hc)::v;
            if (H < rt.nh) {
                STREAM_STEP_BEGIN();
                prod_s<CB, MT, H>(s, qf, cur, min(a.C - H * 256, 256) >> 5, rt, ln, g);
            }
        });
        // ---- online softmax: lane = query ln, keys k0 + 16 j + 4 g + r
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            float tmax = NEG_BIG;
#pragma unroll
            for (int j = 0; j < G::NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float v = k0 + j * 16 + g * 4 + r < a.L ? s[mt][j][r] * a.scale : NEG_BIG;
                    s[mt][j][r] = v;
                    tmax = fmaxf(tmax, v);
                }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16, 64));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
            const float mnew = fmaxf(m[mt], tmax), alpha = __expf(m[mt] - mnew);
            m[mt] = mnew;
            float psum = 0.f;
#pragma unroll
            for (int j = 0; j < G::NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = k0 + j * 16 + g * 4 + r < a.L ? __expf(s[mt][j][r] - mnew) : 0.f;      // a key past L: 0 by index
                    s[mt][j][r] = p;
                    psum += p;
                }
            lsum[mt] = lsum[mt] * alpha + psum;                     // this lane's quarter of the keys: joined once, at the end
#pragma unroll
            for (int ct = 0; ct < G::NCTT; ++ct)
                if (ct * 16 < a.C) o[mt][ct] *= alpha;
        }
        write_tile<CB, MT>(pa, ln, g, [&](int mt, int j, int r) { return s[mt][j][r]; });
        static_for<G::NHM>([&](auto hc) {
            constexpr int H = decltype(hc)::v;
            if (H < rt.nh) {
                STREAM_STEP_BEGIN();
                prod_t<CB, MT, G::NCTT, H * G::NCTH>(o, cur, pa, min(a.C - H * 256, 256) >> 4, rt, ln, g);
            }
        });
    }
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        float lt = lsum[mt];
        lt += __shfl_xor(lt, 16, 64);
        lt += __shfl_xor(lt, 32, 64);
        const float inv = 1.0f / lt;
#pragma unroll
        for (int ct = 0; ct < G::NCTT; ++ct) o[mt][ct] *= inv;
        const int q = wr0 + mt * 16 + ln;
        if (a.lse && g == 0 && q < a.L) a.lse[(long long)bh * a.L + q] = m[mt] + __logf(lt);
    }
    store_own<MT, G::NCTT>(o, a.out + (long long)b * a.L * a.out_ld + hc, a.out_ld, wr0, a.L, 0, a.C, ln, g);
}

// ------------------------------------------------------------------------------------------------ backward: dQ (and D)
template <int CB, int MT>
__global__ __launch_bounds__(NT)
void attn_stream_dq_kernel(StreamArgs a) {
    using G = Geo<CB>;
    __shared__ __attribute__((aligned(16))) char smem[Smem<CB, MT>::BYTES];
    const int tid = threadIdx.x, lane = tid & 63, ln = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bh = blockIdx.y, b = bh / a.heads, hc = (bh - b * a.heads) * a.C, wr0 = blockIdx.x * (64 * MT) + wave * (16 * MT);
    const Rt rt = make_rt(a.L, a.C, G::BN);
    const Opnd Q = make_opnd(a.q + (long long)b * a.L * a.qkv_ld + hc, a.qkv_ld, a.L, a.C);
    const Opnd K = make_opnd(a.k + (long long)b * a.L * a.qkv_ld + hc, a.qkv_ld, a.L, a.C);
    const Opnd V = make_opnd(a.v + (long long)b * a.L * a.qkv_ld + hc, a.qkv_ld, a.L, a.C);
    const Opnd dO = make_opnd(a.d_o + (long long)b * a.L * a.do_ld + hc, a.do_ld, a.L, a.C);
    const Opnd O = make_opnd(a.o + (long long)b * a.L * a.o_ld + hc, a.o_ld, a.L, a.C);
    u32x4 qf[MT][G::KST], dof[MT][G::KST];
    load_own<CB, MT>(qf, Q, wr0, a.L, a.C, ln, g);
    load_own<CB, MT>(dof, dO, wr0, a.L, a.C, ln, g);
    // ---- D[q] = sum_c dO[q][c] O[q][c] from the own dO fragments and O in the same layout: in-lane over the k-steps, then over g
    float dsum[MT], lrow[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int q = wr0 + mt * 16 + ln;
        float acc = 0.f;
#pragma unroll
        for (int ks = 0; ks < G::KST; ++ks) {
            if (ks * 32 < a.C) {
                const u32x4 ov = ldv(O, q < a.L ? (unsigned)(((long long)q * O.ld + ks * 32 + g * 8) * 2) : BUF_OOB);
                float fo[8], fd[8];
                Elem<bf16_t>::unpack(ov, fo); Elem<bf16_t>::unpack(dof[mt][ks], fd);
#pragma unroll
                for (int e = 0; e < 8; ++e) acc += fo[e] * fd[e];
            }
        }
        acc += __shfl_xor(acc, 16, 64);
        acc += __shfl_xor(acc, 32, 64);
        dsum[mt] = acc;
        lrow[mt] = q < a.L ? a.lse[(long long)bh * a.L + q] : 0.f;
        if (g == 0 && q < a.L) a.dvec[(long long)bh * a.L + q] = acc;
    }
    Ring<CB> ring;
    ring.init(smem, tid, rt);
    const unsigned ring0 = lds_addr(smem), pa = ring0 + (unsigned)(3 * G::SLOTB + wave * Smem<CB, MT>::PB);
    const int upt = 3 * rt.nh, nunits = ((a.L + G::BN - 1) / G::BN) * upt;
    auto issue_unit = [&](int uu, int slot) {                       // per key tile: K (score), V (dP), K again (transposed, for dQ)
        const int t = uu / upt, w = uu - t * upt;
        if (w < rt.nh) ring.issue(K, t * G::BN, w, 0, slot, rt);
        else if (w < 2 * rt.nh) ring.issue(V, t * G::BN, w - rt.nh, 0, slot, rt);
        else ring.issue(K, t * G::BN, w - 2 * rt.nh, 1, slot, rt);
    };
    issue_unit(0, 0);
    issue_unit(1, 1);
    f32x4 z[MT][G::NCTT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int ct = 0; ct < G::NCTT; ++ct) z[mt][ct] = (f32x4)(0.f);
    int u = 0, sl = 0;
    for (int k0 = 0; k0 < a.L; k0 += G::BN) {
        f32x4 s[MT][G::NJ], dp[MT][G::NJ];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < G::NJ; ++j) { s[mt][j] = (f32x4)(0.f); dp[mt][j] = (f32x4)(0.f); }
        static_for<G::NHM>([&](auto hc) {
            constexpr int H = decltype(hc)::v;
            if (H < rt.nh) {
                STREAM_STEP_BEGIN();
                prod_s<CB, MT, H>(s, qf, cur, min(a.C - H * 256, 256) >> 5, rt, ln, g);                   // S^T = K_tile Q^T
            }
        });
        static_for<G::NHM>([&](auto hc) {
            constexpr int H = decltype(hc)::v;
            if (H < rt.nh) {
                STREAM_STEP_BEGIN();
                prod_s<CB, MT, H>(dp, dof, cur, min(a.C - H * 256, 256) >> 5, rt, ln, g);                 // dP^T = V_tile dO^T
            }
        });
        write_tile<CB, MT>(pa, ln, g, [&](int mt, int j, int r) {                                         // dS / sqrt(C)
            const bool ok = k0 + j * 16 + g * 4 + r < a.L && wr0 + mt * 16 + ln < a.L;
            const float p = ok ? __expf(s[mt][j][r] * a.scale - lrow[mt]) : 0.f;
            return p * (dp[mt][j][r] - dsum[mt]) * a.scale;
        });
        static_for<G::NHM>([&](auto hc) {
            constexpr int H = decltype(hc)::v;
            if (H < rt.nh) {
                STREAM_STEP_BEGIN();
                prod_t<CB, MT, G::NCTT, H * G::NCTH>(z, cur, pa, min(a.C - H * 256, 256) >> 4, rt, ln, g);   // dQ^T += K_tile^T dS^T
            }
        });
    }
    store_own<MT, G::NCTT>(z, a.dq + (long long)b * a.L * a.dqkv_ld + hc, a.dqkv_ld, wr0, a.L, 0, a.C, ln, g);
}

// ------------------------------------------------------------------------------------------------ backward: dK, dV
// blockIdx.z = the 256-channel half of dK / dV this block produces (C > 256: the accumulators of both halves of both outputs would
// not fit beside the own K and V fragments; the score and dP products, which need all channels, are done by both blocks)
template <int CB, int MT>
__global__ __launch_bounds__(NT)
void attn_stream_dkv_kernel(StreamArgs a) {
    using G = Geo<CB>;
    __shared__ __attribute__((aligned(16))) char smem[Smem<CB, MT>::BYTES];
    const int tid = threadIdx.x, lane = tid & 63, ln = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int bh = blockIdx.y, b = bh / a.heads, hc = (bh - b * a.heads) * a.C, hz = blockIdx.z;
    const int wr0 = blockIdx.x * (64 * MT) + wave * (16 * MT);                                          // wr0: first KEY of the wave
    const Rt rt = make_rt(a.L, a.C, G::BN);
    const Opnd Q = make_opnd(a.q + (long long)b * a.L * a.qkv_ld + hc, a.qkv_ld, a.L, a.C);
    const Opnd K = make_opnd(a.k + (long long)b * a.L * a.qkv_ld + hc, a.qkv_ld, a.L, a.C);
    const Opnd V = make_opnd(a.v + (long long)b * a.L * a.qkv_ld + hc, a.qkv_ld, a.L, a.C);
    const Opnd dO = make_opnd(a.d_o + (long long)b * a.L * a.do_ld + hc, a.do_ld, a.L, a.C);
    u32x4 kf[MT][G::KST], vf[MT][G::KST];
    load_own<CB, MT>(kf, K, wr0, a.L, a.C, ln, g);
    load_own<CB, MT>(vf, V, wr0, a.L, a.C, ln, g);
    Ring<CB> ring;
    ring.init(smem, tid, rt);
    const unsigned ring0 = lds_addr(smem), pa = ring0 + (unsigned)(3 * G::SLOTB + wave * Smem<CB, MT>::PB);
    const int upt = 2 * rt.nh + 2, nunits = ((a.L + G::BN - 1) / G::BN) * upt;
    auto issue_unit = [&](int uu, int slot) {                       // per query tile: Q (score), dO (dP), dO transposed (dV), Q transposed (dK)
        const int t = uu / upt, w = uu - t * upt;
        if (w < rt.nh) ring.issue(Q, t * G::BN, w, 0, slot, rt);
        else if (w < 2 * rt.nh) ring.issue(dO, t * G::BN, w - rt.nh, 0, slot, rt);
        else if (w == 2 * rt.nh) ring.issue(dO, t * G::BN, hz, 1, slot, rt);
        else ring.issue(Q, t * G::BN, hz, 1, slot, rt);
    };
    issue_unit(0, 0);
    issue_unit(1, 1);
    f32x4 zk[MT][G::NCTH], zv[MT][G::NCTH];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int ct = 0; ct < G::NCTH; ++ct) { zk[mt][ct] = (f32x4)(0.f); zv[mt][ct] = (f32x4)(0.f); }
    const int nct = min(a.C - hz * 256, 256) >> 4;
    int u = 0, sl = 0;
    for (int q0 = 0; q0 < a.L; q0 += G::BN) {
        // per-QUERY constants of the tile: lane holds queries q0 + 16 j + 4 g + r
        float lq[G::NJ][4], dq_[G::NJ][4];
#pragma unroll
        for (int j = 0; j < G::NJ; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int q = q0 + j * 16 + g * 4 + r;
                lq[j][r] = q < a.L ? a.lse[(long long)bh * a.L + q] : 0.f;
                dq_[j][r] = q < a.L ? a.dvec[(long long)bh * a.L + q] : 0.f;
            }
        f32x4 s[MT][G::NJ], dp[MT][G::NJ];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < G::NJ; ++j) { s[mt][j] = (f32x4)(0.f); dp[mt][j] = (f32x4)(0.f); }
        static_for<G::NHM>([&](auto hc) {
            constexpr int H = decltype(hc)::v;
            if (H < rt.nh) {
                STREAM_STEP_BEGIN();
                prod_s<CB, MT, H>(s, kf, cur, min(a.C - H * 256, 256) >> 5, rt, ln, g);                   // S = Q_tile K^T
            }
        });
        static_for<G::NHM>([&](auto hc) {
            constexpr int H = decltype(hc)::v;
            if (H < rt.nh) {
                STREAM_STEP_BEGIN();
                prod_s<CB, MT, H>(dp, vf, cur, min(a.C - H * 256, 256) >> 5, rt, ln, g);                  // dP = dO_tile V^T
            }
        });
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int j = 0; j < G::NJ; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const bool ok = q0 + j * 16 + g * 4 + r < a.L && wr0 + mt * 16 + ln < a.L;
                    const float p = ok ? __expf(s[mt][j][r] * a.scale - lq[j][r]) : 0.f;                  // a query past L: 0 by index
                    s[mt][j][r] = p;
                    dp[mt][j][r] = p * (dp[mt][j][r] - dq_[j][r]) * a.scale;
                }
        write_tile<CB, MT>(pa, ln, g, [&](int mt, int j, int r) { return s[mt][j][r]; });                 // P^T
        {
            STREAM_STEP_BEGIN();
            prod_t<CB, MT, G::NCTH, 0>(zv, cur, pa, nct, rt, ln, g);                                      // dV^T += dO_tile^T P
        }
        write_tile<CB, MT>(pa, ln, g, [&](int mt, int j, int r) { return dp[mt][j][r]; });                // dS^T / sqrt(C) (LDS is in order per wave)
        {
            STREAM_STEP_BEGIN();
            prod_t<CB, MT, G::NCTH, 0>(zk, cur, pa, nct, rt, ln, g);                                      // dK^T += Q_tile^T dS
        }
    }
    const int cend = min(a.C, hz * 256 + 256);
    store_own<MT, G::NCTH>(zv, a.dv + (long long)b * a.L * a.dqkv_ld + hc, a.dqkv_ld, wr0, a.L, hz * 256, cend, ln, g);
    store_own<MT, G::NCTH>(zk, a.dk + (long long)b * a.L * a.dqkv_ld + hc, a.dqkv_ld, wr0, a.L, hz * 256, cend, ln, g);
}

// C: the width of one third of the packed buffer = heads * d.  heads = 1 is the single-head contract, with its status codes.
static int check_stream(const void* qkv, long long ld, int B, int L, int C, int heads, int dtype) {
    if (!qkv) return DDPM_ERR_NULL;
    if (dtype != DDPM_BF16) return DDPM_ERR_DTYPE;
    if (B <= 0 || L <= 0 || C <= 0 || heads < 1 || C % heads || (long long)B * heads > 65535) return DDPM_ERR_SHAPE;      // blockIdx.y = (b, h)
    const int d = C / heads;
    if (d > 512 || d % 32 || ld < 3LL * C) return DDPM_ERR_SHAPE;
    if (!aligned16(qkv) || ld % 8) return DDPM_ERR_ALIGN;
    if ((long long)L * ld * 2 > BUF_OOB) return DDPM_ERR_SHAPE;
    return DDPM_OK;
}

template <class K>
static int launch(K kernel, dim3 grid, hipStream_t st, const StreamArgs& a) {
    hipLaunchKernelGGL(kernel, grid, dim3(NT), 0, st, a);
    return check_launch();
}

// the forward of `heads` heads of width C / heads each; bucket and MT follow the HEAD's width
static int stream_fwd(const void* qkv, long long ld, void* out, long long out_ld, float* lse, int B, int L, int C, int heads, float scale,
                      int dtype, void* stream) {
    int rc = check_stream(qkv, ld, B, L, C, heads, dtype);
    if (rc) return rc;
    if (!out) return DDPM_ERR_NULL;
    if (!aligned16(out) || out_ld % 8) return DDPM_ERR_ALIGN;
    if (out_ld < C) return DDPM_ERR_SHAPE;
    const int d = C / heads, BH = B * heads;
    StreamArgs a; memset(&a, 0, sizeof(a));
    a.q = (const bf16_t*)qkv; a.k = a.q + C; a.v = a.q + 2 * C; a.qkv_ld = ld;
    a.out = (bf16_t*)out; a.out_ld = out_ld; a.lse = lse;
    a.B = B; a.L = L; a.C = d; a.heads = heads; a.scale = scale;
    hipStream_t st = (hipStream_t)stream;
    if (d <= 64) return launch(&attn_stream_fwd_kernel<64, 2>, dim3((L + 127) / 128, BH), st, a);
    if (d <= 128) return launch(&attn_stream_fwd_kernel<128, 2>, dim3((L + 127) / 128, BH), st, a);
    if (d <= 256) return launch(&attn_stream_fwd_kernel<256, 2>, dim3((L + 127) / 128, BH), st, a);
    return launch(&attn_stream_fwd_kernel<512, 1>, dim3((L + 63) / 64, BH), st, a);
}

static int stream_bwd(const void* qkv, long long ld, const void* o, long long o_ld, const void* d_o, long long do_ld, const float* lse,
                      float* dvec, void* dqkv, long long dqkv_ld, int B, int L, int C, int heads, float scale, int dtype, void* stream) {
    int rc = check_stream(qkv, ld, B, L, C, heads, dtype);
    if (rc) return rc;
    if (!o || !d_o || !lse || !dvec || !dqkv) return DDPM_ERR_NULL;
    if (!aligned16(o) || !aligned16(d_o) || !aligned16(dqkv) || o_ld % 8 || do_ld % 8 || dqkv_ld % 8 || dqkv_ld < 3LL * C) return DDPM_ERR_ALIGN;
    if (o_ld < C || do_ld < C || (long long)L * o_ld * 2 > BUF_OOB || (long long)L * do_ld * 2 > BUF_OOB) return DDPM_ERR_SHAPE;
    const int d = C / heads, BH = B * heads;
    StreamArgs a; memset(&a, 0, sizeof(a));
    a.q = (const bf16_t*)qkv; a.k = a.q + C; a.v = a.q + 2 * C; a.qkv_ld = ld;
    a.o = (const bf16_t*)o; a.o_ld = o_ld; a.d_o = (const bf16_t*)d_o; a.do_ld = do_ld;
    a.dq = (bf16_t*)dqkv; a.dk = a.dq + C; a.dv = a.dq + 2 * C; a.dqkv_ld = dqkv_ld;
    a.lse = const_cast<float*>(lse); a.dvec = dvec;
    a.B = B; a.L = L; a.C = d; a.heads = heads; a.scale = scale;
    hipStream_t st = (hipStream_t)stream;
    const dim3 g2((L + 127) / 128, BH), g1((L + 63) / 64, BH), g1z((L + 63) / 64, BH, 2);
    if (d <= 64) { rc = launch(&attn_stream_dq_kernel<64, 2>, g2, st, a); return rc ? rc : launch(&attn_stream_dkv_kernel<64, 2>, g2, st, a); }
    if (d <= 128) { rc = launch(&attn_stream_dq_kernel<128, 2>, g2, st, a); return rc ? rc : launch(&attn_stream_dkv_kernel<128, 2>, g2, st, a); }
    if (d <= 256) { rc = launch(&attn_stream_dq_kernel<256, 1>, g1, st, a); return rc ? rc : launch(&attn_stream_dkv_kernel<256, 1>, g1, st, a); }
    rc = launch(&attn_stream_dq_kernel<512, 1>, g1, st, a);
    return rc ? rc : launch(&attn_stream_dkv_kernel<512, 1>, g1z, st, a);
}

}  // namespace

// Forward at any token count:  out[b][i][:] = sum_j softmax_j(q_i . k_j * scale) v_j ;  lse[b][i] = log sum_j exp(q_i . k_j * scale)
// (optional).  qkv: packed [B][L][ld] with q at channel 0, k at C, v at 2C.  bf16; any L >= 1 with L * ld * 2 within the buffer
// descriptors' range; C <= 512, C % 32 == 0.  (The heads = 1 case of the multi-head entry below: the same code.)
extern "C" int ddpm_attention_stream_fwd(const void* qkv, long long ld, void* out, long long out_ld, float* lse, int B, int L, int C,
                                         float scale, int dtype, void* stream) {
    return stream_fwd(qkv, ld, out, out_ld, lse, B, L, C, 1, scale, dtype, stream);
}

// Backward of the above given the saved output o, its gradient d_o and lse: writes dq / dk / dv into the packed gradient buffer
// dqkv [B][L][dqkv_ld] (dq at channel 0, dk at C, dv at 2C).  dvec: [B][L] fp32 workspace (receives D = rowsum(dO o O)).
// Two kernels, each output element produced by one workgroup in a fixed order: a repeated call is bit-identical.
extern "C" int ddpm_attention_stream_bwd(const void* qkv, long long ld, const void* o, long long o_ld, const void* d_o, long long do_ld,
                                         const float* lse, float* dvec, void* dqkv, long long dqkv_ld, int B, int L, int C, float scale,
                                         int dtype, void* stream) {
    return stream_bwd(qkv, ld, o, o_ld, d_o, do_ld, lse, dvec, dqkv, dqkv_ld, B, L, C, 1, scale, dtype, stream);
}

// Multi-head: d = C / heads, head h of q, k, v = channels [h d, (h + 1) d) of its third of the packed buffer (qkv.chunk(3) and then a
// split of each third into heads), and of out, o, d_o and the thirds of dqkv likewise:
//     out[b][i][h d + c] = sum_j softmax_j(q_h[b][i] . k_h[b][j] * scale) v_h[b][j][c]
// lse, dvec: [B][heads][L] fp32.  The caller passes scale (1 / sqrt(d) for the usual attention).  heads >= 1, C % heads == 0,
// d % 32 == 0, d <= 512 (any C), B * heads <= 65535; everything else as the pair above, which is its heads = 1 case.  One launch per
// kernel over B * heads problems: a head reads and writes only its own [L][d] of every operand and output.
extern "C" int ddpm_attention_mh_fwd(const void* qkv, long long ld, void* out, long long out_ld, float* lse, int B, int L, int C, int heads,
                                     float scale, int dtype, void* stream) {
    return stream_fwd(qkv, ld, out, out_ld, lse, B, L, C, heads, scale, dtype, stream);
}

extern "C" int ddpm_attention_mh_bwd(const void* qkv, long long ld, const void* o, long long o_ld, const void* d_o, long long do_ld,
                                     const float* lse, float* dvec, void* dqkv, long long dqkv_ld, int B, int L, int C, int heads,
                                     float scale, int dtype, void* stream) {
    return stream_bwd(qkv, ld, o, o_ld, d_o, do_ld, lse, dvec, dqkv, dqkv_ld, B, L, C, heads, scale, dtype, stream);
}
