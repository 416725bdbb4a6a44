// Universal MFMA GEMM / implicit-GEMM convolution for gfx950 (MI355X).
//
//   C[b][m][n] = alpha * sum_k A[b][m][k] * B[b][n][k]   (+ fused epilogue)
//
// One kernel template covers every contraction on the DDPM hot path (SURVEY.md §8a rows a2,a3,a4,a5,a7,a9,
// and their dgrad / wgrad):
//   * 3x3 / 1x1 convolution forward and dgrad over NHWC activations: the A operand is an implicit im2col
//     gather (rows = output pixels, k = (r,s,c)), with TF-SAME stride-2, nearest-2x-upsample and
//     dilated (transposed-conv) index maps folded into the tile loader — no pad / upsample / cat tensors;
//   * wgrad: both operands are read "transposed" (reduction index is the slow memory index) and the
//     epilogue scatters fp32 atomics straight into the [Cout][Cin][R][S] gradient;
//   * Linear layers and the attention matmuls (QK^T, PV and their four backward products) as batched GEMMs.
//
// Tiling: 128x128 block tile, 256 threads = 4 waves (2x2), each wave 64x64 = 2x2 MFMA 32x32 accumulators
// (64 accumulator registers), K-step BK = 8 vectors of 16 bytes (64 bf16 / 32 fp32), double-buffered LDS
// (register-staged: global -> VGPR -> LDS, loads of step s+1 in flight while step s computes).
//   bf16: v_mfma_f32_32x32x16_bf16 (8 bf16 per lane per operand, fp32 accumulate)
//   fp32: v_mfma_f32_32x32x2_f32   (exact fp32 — the 1e-3 parity path; lanes hold 4 consecutive k, the
//         k-permutation is the same for A and B so the contraction is unchanged)
// k-contiguous operands go HBM/L2 -> LDS directly (global_load_lds_dwordx4, no VGPR staging); LDS rows are 128 bytes,
// unpadded, with the 16-byte chunks XOR-swizzled by (row & 7) via the per-lane SOURCE address, so the LDS image
// stays lane-linear for the DMA and the 16-lane groups of ds_read_b128 hit distinct 16-B slots.
#include "common.h"
#include <string.h>
#include <stdlib.h>

struct MatDesc {
    const void* p;
    long long batch_stride;   // elements
    long long ld;             // pitch (elements) of the slow memory index
    int trans;                // 0: slow index = M/N index, fast (contiguous) = K.  1: slow = K, fast = M/N
    int conv;                 // 1: slow = output pixel, fast = (r*S+s)*C + c gathered from NHWC (pixel pitch ld)
    int n_slow, n_fast;       // logical extents (rows beyond are zero)
    unsigned extent_bytes;    // bytes addressable from (p + batch*batch_stride): bound of the buffer descriptor (< 2 GiB)
    int H, W, C, Ho, Wo, R, S, stride, pad_t, pad_l;
    int conv_batches;         // conv: images in the NHWC tensor (extent = conv_batches*H*W pixels)
    int sh;                   // 1 when the virtual input grid is 2x the stored one (upsample or dilation)
    int dmask;                // 1 for dilation-2 (only even virtual coordinates exist), else 0
    FastDiv dHoWo, dWo, dC, dS;
    // Parity-phase form of the dilation-2 conv (the data gradient of a stride-2 conv), set by the host when the geometry allows it: the output rows
    // are walked PHASE-MAJOR — m = phase * Mp + ((b * Hh + h') * Wh + w'), output pixel (2h' + a, 2w' + bb) — so that all rows of a 128-row tile
    // have the same coordinate parities and hence the same non-zero taps (1, 2, 2 or 4 of the 9): the K loop visits those only and the
    // zero-dilated three quarters of the operand are never fetched or multiplied.
    int phase, Hh, Wh, Mp, spt;       // spt = K-steps per tap (C / BK)
    FastDiv dMp, dHhWh, dWh, dSpt;
};

// phase-major row m -> phase id, image, output pixel.  Phase ids in the order 4-tap, 2-tap, 1-tap, 2-tap: blocks
// are dispatched in id order and a CU holds two of them, so the k-th and (k + half)-th tiles share a CU — 4 + 1 and 2 + 2 taps.
// (a coordinate whose parity equals the pad's has the two even taps r = 0, 2 of a 3-tap axis, the other parity the single odd one)
__device__ __forceinline__ void phase_parity(const MatDesc& d, int ph, int& a, int& bb) {
    a = (d.pad_t & 1) ^ (ph < 2 ? 0 : 1);
    bb = (d.pad_l & 1) ^ ((ph == 0 || ph == 3) ? 0 : 1);
}
__device__ __forceinline__ void phase_decode(const MatDesc& d, int m, int& ph, int& b, int& y, int& x) {
    ph = (int)fdiv((unsigned)m, d.dMp);
    const unsigned q = (unsigned)m - (unsigned)ph * (unsigned)d.Mp;
    const unsigned bq = fdiv(q, d.dHhWh);
    const unsigned rem = q - bq * (unsigned)(d.Hh * d.Wh);
    const unsigned hh = fdiv(rem, d.dWh), wh = rem - hh * (unsigned)d.Wh;
    int a, bb;
    phase_parity(d, ph, a, bb);
    b = (int)bq; y = 2 * (int)hh + a; x = 2 * (int)wh + bb;
}

struct Epilogue {
    void* out;
    long long out_batch_stride, ldc;
    int mode;                 // 0 store T | 1 store f32 | 2 atomic-add f32 | 3 store f32 NCHW | 4 packed wgrad (atomic when accumulate)
    float alpha;
    const float* bias;        // [N] or null
    const float* rowbias;     // [M / rows_per_group][rowbias_ld] or null (time bias per sample)
    long long rowbias_ld;
    FastDiv dgroup;           // rows per group (H*W of the output)
    const void* residual;     // T, [M][res_ld] or null
    long long res_ld, res_batch_stride;
    int accumulate;           // modes 0/1: out += result
    int Cpad, Creal, RS;      // modes 4 / 5: col = tap*Cpad + c -> packed gradient dst[(row*RS + tap)*Creal + c]
    long long slab_stride;    // mode 5: split s STORES its partial into copy s (out + s*slab_stride floats); the caller sums
    FastDiv dCpad;
    FastDiv dHW;              // mode 3: row -> (b, pixel)
    int HW;
    int vec_ok;               // out / residual pointers and pitches allow 16-byte vector access
    float* splitk_ws;         // split-K slabs [tile][split][128*128] fp32 (modes 0/1/3 with gridDim.y > 1), else null
    unsigned* splitk_cnt;     // per-tile arrival counters, zero on entry, reset to zero by the last arriver
};

template <typename T> struct Mma;
template <> struct Mma<bf16_t> {
    typedef __bf16 frag_t __attribute__((ext_vector_type(8)));
    static constexpr int KF = 16;    // k covered per fragment step
    __device__ static __forceinline__ void run(const u32x4& a, const u32x4& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(frag_t, a), __builtin_bit_cast(frag_t, b), c, 0, 0, 0);
    }
};
template <> struct Mma<float> {
    static constexpr int KF = 8;
    __device__ static __forceinline__ void run(const u32x4& a, const u32x4& b, f32x16& c) {
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), c, 0, 0, 0);
        c = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), c, 0, 0, 0);
    }
};

constexpr int TILE = 128;      // BM == BN
constexpr int NTHREADS = 256;  // 4-wave blocks; the 8-wave variant (NW = 8) uses 512
constexpr int ROW_BYTES = 128; // LDS row pitch: 128 B of K data, unpadded (XOR-swizzled chunks)
constexpr int NVEC = 4;        // 16-byte vectors per thread per operand per K-step

// LDS operand tile: 128 rows x 128 bytes (64 bf16 / 32 fp32 of K), UNPADDED, with the 16-byte chunk index XOR-swizzled
// by ((row>>1) & 7): element (row, chunk c) lives at row*128 + ((c ^ ((row>>1)&7)) * 16).  Two consecutive rows span one
// 256-byte bank row, so the key must be distinct over the 8 even (odd) rows of each ds_read_b128 16-lane group
// ({0-3,12-15,20-27} / {4-11,16-19,28-31}): (row>>1)&7 is, row&7 is not (rows 12 and 20 would collide).  Rows stay
// contiguous, which the LDS-DMA loads require.
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * ROW_BYTES + ((chunk ^ ((row >> 1) & 7)) << 4); }

// Per-thread loader state for one operand tile (TILE rows x BK k).  All global reads go through a raw buffer descriptor
// (base = operand pointer of this batch, num_records = its extent): addressing is one 32-bit byte offset per vector and
// the hardware range check returns ZEROS for any offset >= num_records — padded taps, K-tails and rows beyond the matrix
// simply use the offset BUF_OOB (verified on gfx950 also for the direct-to-LDS form: scripts/probes/buffer_lds_oob.hip).
//  !TRANS (memory is k-contiguous): `buffer_load_dwordx4 ... lds` — HBM/L2 -> LDS without touching VGPRs.  Lane l of wave w
//          fetches, for i = 0..3, row w*8 + l/8 + 32 i, PHYSICAL chunk l%8, i.e. logical k-chunk (l%8) ^ ((row>>1)&7):
//          the swizzle is applied on the per-lane SOURCE offset, the LDS image stays lane-linear.
//   TRANS (k is the slow memory index): each thread owns a 4(k) x VEC(m) block — k-quad kq = tid % (BK/4) fastest over
//          lanes, m-group ng = tid / (BK/4) — loads its 4 k-rows as 16-byte vectors, transposes in registers and writes
//          VEC k-contiguous 4-element runs (ds_write_b64 bf16 / ds_write_b128 fp32) into the swizzled image.

// PH: the parity-phase conv form is compiled in.  CV = false: the operand is never an implicit-im2col view (the B side of the k-contiguous
// products is always a plain weight matrix) — its gather arithmetic is left out of the block prologue.
template <typename T, bool TRANS, int NW = 4, int ROWS = 128, bool PH = false, bool CV = true>
struct Loader {
    static constexpr int NT = NW * 64;                       // threads per block
    static constexpr int NV = ROWS * 8 / NT;                 // 16-byte vectors per thread per operand per K-step
    static_assert(ROWS == 128 || !TRANS, "only the k-contiguous path is built for the 64-row tile");
    static constexpr int VEC = Elem<T>::VEC;
    static constexpr int BK = 8 * VEC;
    static constexpr int KQ = BK / 4;
    static constexpr int ES = (int)sizeof(T);
    static constexpr bool TR16 = TRANS && sizeof(T) == 2;    // k-strided bf16 operand: LDS-DMA + ds_read_b64_tr_b16
    static constexpr bool DMA = !TRANS || TR16;              // operand staged HBM/L2 -> LDS without VGPRs
    static_assert(NW == 4 || DMA, "the register-transposed path is laid out for 256 threads");

    const MatDesc& d;
    __amdgpu_buffer_rsrc_t rsrc;
    int tile0;
    int kv, wave, row0;           // !TRANS: logical k-chunk, wave id, first tile row
    int kvoff, kuni;              // !TRANS conv: byte offset of this lane's chunk inside a K-step; 1 when a K-step never straddles two taps (C % BK == 0)
    int kq, ng;                   // TRANS
    int roff[NV];               // !TRANS: byte offset of the row (plain; BUF_OOB when the row is outside) or of pixel (b, y0, x0) (conv)
    unsigned tapmask[NV];       // !TRANS conv without up/down-scaling: bit (r*S+s) set when the tap is inside the image
    int tr, ts, tc; unsigned foff;   // TRANS: fixed tap/channel (conv) or fixed byte offset along the fast index (plain, BUF_OOB if outside)
    int krow0;                    // TRANS bf16 (LDS-DMA of the m-major image): first k-row of this thread (tid>>4), +16 per vector
    int ph_py, ph_px;             // !TRANS parity-phase conv: parity of (y - pad_t), (x - pad_l) of this tile's rows; -1 otherwise

    __device__ __forceinline__ Loader(const MatDesc& d_, int batch, int tile0_, int tid) : d(d_) {
        rsrc = buffer_rsrc(reinterpret_cast<const T*>(d.p) + (long long)batch * d.batch_stride, (unsigned)d.extent_bytes);
        tile0 = tile0_;
        if (!TRANS) {
            row0 = tid >> 3;
            wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            kv = (tid & 7) ^ ((row0 >> 1) & 7);
            kvoff = kv * VEC * ES;
            kuni = (CV && d.conv && (d.sh == 0 || (PH && d.phase)) && d.C % BK == 0) ? 1 : 0;
            ph_py = ph_px = -1;
            if (PH && d.conv && d.phase) {
                // every row of the tile is in one phase (Mp is a multiple of the tile height): the parities are block-uniform
                int a, bb;
                phase_parity(d, (int)fdiv((unsigned)__builtin_amdgcn_readfirstlane(tile0), d.dMp), a, bb);
                ph_py = (a - d.pad_t) & 1; ph_px = (bb - d.pad_l) & 1;
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int m = tile0 + row0 + (NT / 8) * i;
                    int ph, b, y, x;
                    phase_decode(d, m, ph, b, y, x);
                    const int y0 = y - d.pad_t, x0 = x - d.pad_l;           // virtual (zero-dilated) coordinates of tap (0, 0)
                    // tap (r, s) reads the STORED pixel ((y0 + r) / 2, (x0 + s) / 2) when both sums are even and inside; relative to the
                    // pixel (y0 >> 1, x0 >> 1) that is ((r + py) >> 1, (s + px) >> 1) — the same for every row of the tile
                    const int yb = y0 >> 1, xb = x0 >> 1;
                    roff[i] = (int)((((long long)(b * d.H + yb) * d.W + xb) * d.ld) * ES);
                    unsigned mk = 0;
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int s = 0; s < 3; ++s) {
                            const unsigned sy = (unsigned)(yb + ((r + ph_py) >> 1)), sx = (unsigned)(xb + ((s + ph_px) >> 1));
                            const bool ok = r < d.R && s < d.S && (r & 1) == ph_py && (s & 1) == ph_px && sy < (unsigned)d.H && sx < (unsigned)d.W;
                            mk |= ok ? 1u << (r * d.S + s) : 0u;
                        }
                    tapmask[i] = mk;
                }
            } else if constexpr (!CV) {
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const int m = tile0 + row0 + (NT / 8) * i;
                    roff[i] = m < d.n_slow ? (int)((long long)m * d.ld * ES) : (int)BUF_OOB;
                    tapmask[i] = 0u;
                }
            } else
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int m = tile0 + row0 + (NT / 8) * i;
                const bool valid = m < d.n_slow;
                // both addressing forms are computed and SELECTED (no divergent stores into the state arrays -> registers)
                int b, y0, x0;
                decode_pixel(valid ? m : 0, b, y0, x0);
                const int conv_off = (int)((((long long)(b * d.H + y0) * d.W + x0) * d.ld) * ES);
                const int plain_off = valid ? (int)((long long)m * d.ld * ES) : (int)BUF_OOB;
                // taps inside the image: rows r in [max(0,-y0), min(R, H-y0)), columns likewise (closed form, R,S <= 5)
                const int rlo = min(max(-y0, 0), d.R), rhi = min(max(d.H - y0, 0), d.R);
                const int slo = min(max(-x0, 0), d.S), shi = min(max(d.W - x0, 0), d.S);
                const unsigned vy = ((1u << rhi) - 1u) & ~((1u << rlo) - 1u), vx = ((1u << shi) - 1u) & ~((1u << slo) - 1u);
                unsigned mk = 0;
#pragma unroll
                for (int r = 0; r < 5; ++r) mk |= ((vy >> r) & 1u) ? vx << (r * d.S) : 0u;
                roff[i] = d.conv ? conv_off : plain_off;
                tapmask[i] = (d.conv && valid) ? mk : 0u;
            }
        } else {
            kq = tid % KQ; ng = tid / KQ;
            wave = __builtin_amdgcn_readfirstlane(tid >> 6);
            krow0 = tid >> 4;
            // bf16: thread owns PHYSICAL 16-byte chunk tid&15 of k-rows krow0 + 16 i, i.e. logical chunk (tid&15) ^ ((krow&3)<<2)
            const int f = TR16 ? tile0 + (((tid & 15) ^ ((krow0 & 3) << 2)) * VEC) : tile0 + ng * VEC;
            const bool fvalid = f < d.n_fast;
            foff = fvalid ? (unsigned)(f * ES) : BUF_OOB;
            if (d.conv) {
                unsigned tap = fdiv((unsigned)(fvalid ? f : 0), d.dC);
                tc = fvalid ? f - (int)tap * d.C : -1;      // tc < 0 marks "outside"
                tr = (int)fdiv(tap, d.dS); ts = (int)tap - tr * d.S;
            }
        }
    }

    __device__ __forceinline__ void decode_pixel(int m, int& b, int& y0, int& x0) const {
        unsigned bb = fdiv((unsigned)m, d.dHoWo);
        unsigned rem = (unsigned)m - bb * (unsigned)(d.Ho * d.Wo);
        unsigned oy = fdiv(rem, d.dWo);
        unsigned ox = rem - oy * (unsigned)d.Wo;
        b = (int)bb; y0 = (int)oy * d.stride - d.pad_t; x0 = (int)ox * d.stride - d.pad_l;
    }

    // byte offset of the 16-byte vector at virtual pixel (y0+r, x0+s), channel c — or BUF_OOB
    __device__ __forceinline__ unsigned gather_off(int b, int y0, int x0, int r, int s, int c) const {
        unsigned uy = (unsigned)(y0 + r), ux = (unsigned)(x0 + s);
        bool ok = ((uy | ux) & (unsigned)d.dmask) == 0;
        uy >>= d.sh; ux >>= d.sh;
        ok = ok && uy < (unsigned)d.H && ux < (unsigned)d.W;
        const unsigned off = (unsigned)(((b * d.H + (int)uy) * d.W + (int)ux) * (int)d.ld + c) * ES;
        return ok ? off : BUF_OOB;
    }

    // !TRANS: enqueue the direct-to-LDS loads of the K-step starting at k0 into `tile`
    __device__ __forceinline__ void issue(int k0, int k_end, char* tile) const {
        const int k = k0 + kv * VEC;
        const bool kok = k < k_end;
        unsigned off[NV];
        if (kuni) {
            // C is a multiple of the K-step: the step lies inside ONE tap, so tap, channel and tap offset are wave-uniform
            // (SALU) and a lane is left with the mask test and one add per row — the per-lane divisions below cost ~250 clk
            // per call, fully exposed with one wave per SIMD (scripts/g64_timeline.py).
            const int k0u = __builtin_amdgcn_readfirstlane(k0);
            const unsigned tapu = fdiv((unsigned)k0u, d.dC);
            const int cu = k0u - (int)tapu * d.C;
            int ru = (int)fdiv(tapu, d.dS), su = (int)tapu - ru * d.S;
            if (PH && ph_py >= 0) { ru = (ru + ph_py) >> 1; su = (su + ph_px) >> 1; }     // parity-phase conv: offsets on the stored (undilated) grid
            const int tapoff = ((ru * d.W + su) * (int)d.ld + cu) * ES;
            const unsigned tb = k0u < k_end ? tapu : 31u;           // K is a multiple of the step here: no partial tail
#pragma unroll
            for (int i = 0; i < NV; ++i) off[i] = ((tapmask[i] >> tb) & 1u) ? (unsigned)(roff[i] + kvoff + tapoff) : BUF_OOB;
        } else if (CV && d.conv) {
            unsigned tap = fdiv((unsigned)k, d.dC);
            const int c = k - (int)tap * d.C;
            const int r = (int)fdiv(tap, d.dS), s = (int)tap - r * d.S;
            if (d.sh == 0) {
                const int tapoff = ((r * d.W + s) * (int)d.ld + c) * ES;
                tap = kok ? tap : 31u;                          // bit 31 is never set: K-tail reads zeros
#pragma unroll
                for (int i = 0; i < NV; ++i) off[i] = ((tapmask[i] >> tap) & 1u) ? (unsigned)(roff[i] + tapoff) : BUF_OOB;
            } else {
#pragma unroll
                for (int i = 0; i < NV; ++i) {        // up/down-scaled maps (6 convs per pass): decode on the fly
                    const int m = tile0 + row0 + (NT / 8) * i;
                    int b, y0, x0;
                    decode_pixel(m < d.n_slow ? m : 0, b, y0, x0);
                    off[i] = (kok && m < d.n_slow) ? gather_off(b, y0, x0, r, s, c) : BUF_OOB;
                }
            }
        } else {
            const unsigned koff = kok ? (unsigned)(k * ES) : BUF_OOB;
#pragma unroll
            for (int i = 0; i < NV; ++i) off[i] = (unsigned)roff[i] + koff;     // BUF_OOB + small stays out of range
        }
#pragma unroll
        for (int i = 0; i < NV; ++i)
            LDS_DMA16(rsrc, tile + (wave * 8 + (NT / 8) * i) * ROW_BYTES, off[i], 0);
    }

    // TRANS bf16: LDS-DMA of the operand AS STORED (k-rows of 128 m-elements = 256 bytes, 64 rows per K-step) with the
    // 16-byte chunks XOR-swizzled by (krow & 3) << 2 on the source side; fragments are then formed by the hardware
    // transpose read (ds_read_b64_tr_b16: in each 16-lane group lanes 4r..4r+3 supply row r, lane c receives column c).
    __device__ __forceinline__ void issue_tr(int k0, int k_end, char* tile) const {
        unsigned off[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int k = k0 + krow0 + (NT / 16) * i;
            if (d.conv) {
                int b, y0, x0;
                decode_pixel(k < k_end ? k : 0, b, y0, x0);
                off[i] = (tc >= 0 && k < k_end) ? gather_off(b, y0, x0, tr, ts, tc) : BUF_OOB;
            } else {
                off[i] = k < k_end ? (unsigned)((long long)k * d.ld * ES) + foff : BUF_OOB;
            }
        }
#pragma unroll
        for (int i = 0; i < NV; ++i)
            LDS_DMA16(rsrc, tile + (wave * 64 + NT * i) * 16, off[i], 0);
    }

    // TRANS: fetch this thread's 4 k-rows of the K-step starting at k0
    __device__ __forceinline__ void load(int k0, int k_end, u32x4 (&v)[NV]) const {
        const int kb = k0 + kq * 4;
        if (d.conv) {
            int b, y0, x0;
            decode_pixel(kb < k_end ? kb : 0, b, y0, x0);
            const int xend = d.Wo * d.stride - d.pad_l, yend = d.Ho * d.stride - d.pad_t;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const bool ok = tc >= 0 && kb + i < k_end;
                const unsigned o = ok ? gather_off(b, y0, x0, tr, ts, tc) : BUF_OOB;
                v[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o, 0, 0));
                x0 += d.stride;                                   // next output pixel (row-major over b, oy, ox)
                if (x0 == xend) { x0 = -d.pad_l; y0 += d.stride; if (y0 == yend) { y0 = -d.pad_t; ++b; } }
            }
        } else {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int k = kb + i;
                const unsigned o = k < k_end ? (unsigned)((long long)k * d.ld * ES) + foff : BUF_OOB;
                v[i] = __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(rsrc, o, 0, 0));
            }
        }
    }

    // TRANS: register-transpose the 4 x VEC block and write it into the swizzled K-contiguous tile
    __device__ __forceinline__ void store(char* tile, const u32x4 (&v)[NV]) const {
        if (sizeof(T) == 2) {
#pragma unroll
            for (int dd = 0; dd < 4; ++dd) {            // dword dd of each vector holds m = 2dd (low half) and 2dd+1 (high half)
                const unsigned a0 = v[0][dd], a1 = v[1][dd], a2 = v[2][dd], a3 = v[3][dd];
                uint2 even, odd;
                even.x = (a0 & 0xffffu) | (a1 << 16); even.y = (a2 & 0xffffu) | (a3 << 16);
                odd.x = (a0 >> 16) | (a1 & 0xffff0000u); odd.y = (a2 >> 16) | (a3 & 0xffff0000u);
                *reinterpret_cast<uint2*>(tile + lds_off(ng * 8 + 2 * dd, kq >> 1) + (kq & 1) * 8) = even;
                *reinterpret_cast<uint2*>(tile + lds_off(ng * 8 + 2 * dd + 1, kq >> 1) + (kq & 1) * 8) = odd;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u32x4 w; w.x = v[0][j]; w.y = v[1][j]; w.z = v[2][j]; w.w = v[3][j];
                *reinterpret_cast<u32x4*>(tile + lds_off(ng * 4 + j, kq)) = w;
            }
        }
    }
};

// ---------------------------------------------------------------------------------------------- epilogue
// The accumulators are staged through LDS as fp32 [128][CS_LD] so that every global access of the epilogue is a
// 16-byte vector along n (bias / time-bias / residual reads and the output write are fully coalesced).
constexpr int CS_LD = TILE + 4;

// `rowmap(rl)` gives the global output row of staged row rl (or -1 to skip it); NROWS rows are staged in `cs`.
// per-thread bias vector of the row epilogue (thread tid owns output columns col0g + (tid % VPR) * VO ...): loaded early
// by the kernels so that its latency hides under the accumulator staging
template <typename OutT, int NT, int TN = 128>
__device__ __forceinline__ void epilogue_bias(const Epilogue& ep, int col0g, int N, int tid, float (&bias)[16 / (int)sizeof(OutT)]) {
    constexpr int VO = 16 / (int)sizeof(OutT), VPR = TN / VO;
    const int col = col0g + (tid % VPR) * VO;
#pragma unroll
    for (int j = 0; j < VO; ++j) bias[j] = (ep.bias && col + j < N) ? ep.bias[col + j] : 0.f;
}

// Row epilogue in two phases per batch of U rows: load() issues every global read of the batch (time bias, residual,
// accumulate target), finish() consumes them together with the staged accumulators.  The kernels call load(0) BEFORE they
// stage the accumulators through LDS, so that first (usually only) batch's memory latency hides under the staging.
template <typename T, typename OutT, int NT, int NROWS, int TN, typename RowMap>
struct RowEpilogue {
    static constexpr int VO = 16 / (int)sizeof(OutT);     // output elements per 16-byte vector
    static constexpr int VPR = TN / VO;                    // vectors per tile row
    static constexpr int LD = TN + 4;                      // staging pitch
    static constexpr int PER_THREAD = (NROWS * VPR + NT - 1) / NT;
    static constexpr int ROWS_PER_PASS = NT / VPR;
    static constexpr int U = PER_THREAD < 4 ? PER_THREAD : 4;
    static constexpr bool SAME = sizeof(T) == sizeof(OutT);
    const Epilogue& ep;
    RowMap rowmap;
    int N, cv, r0, col;
    bool live, fast;
    OutT* outb;
    const T* resb;
    int rows[U];
    float rbv[U][VO];
    u32x4 resv[U], accv[U];

    __device__ __forceinline__ RowEpilogue(const Epilogue& ep_, int batch, RowMap rm, int col0g, int N_, int tid) : ep(ep_), rowmap(rm), N(N_) {
        cv = tid % VPR; r0 = tid / VPR;
        col = col0g + cv * VO;
        live = col < N;
        fast = col + VO <= N && ep.vec_ok;
        outb = reinterpret_cast<OutT*>(ep.out) + (long long)batch * ep.out_batch_stride;
        resb = ep.residual ? reinterpret_cast<const T*>(ep.residual) + (long long)batch * ep.res_batch_stride : nullptr;
    }
    __device__ __forceinline__ void load(int i0) {
        if (!live) return;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int rl = r0 + (i0 + u) * ROWS_PER_PASS;
            const int row = (i0 + u < PER_THREAD && rl < NROWS) ? rowmap(rl) : -1;
            rows[u] = row;
            if (row < 0) continue;
            if (ep.rowbias) {
                const float* rb = ep.rowbias + (long long)fdiv((unsigned)row, ep.dgroup) * ep.rowbias_ld + col;
#pragma unroll
                for (int j = 0; j < VO; ++j) rbv[u][j] = (col + j < N) ? rb[j] : 0.f;
            }
            if (fast) {
                if (resb && SAME) resv[u] = ldg16(resb + (long long)row * ep.res_ld + col);
                if (ep.accumulate) accv[u] = ldg16(outb + (long long)row * ep.ldc + col);
            }
        }
    }
    __device__ __forceinline__ void finish(int i0, const float* cs, const float (&bias)[VO]) {
        if (!live) return;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int row = rows[u];
            if (row < 0) continue;
            const int rl = r0 + (i0 + u) * ROWS_PER_PASS;
            float v[VO];
#pragma unroll
            for (int j = 0; j < VO; j += 4) {
                const f32x4 t = *reinterpret_cast<const f32x4*>(cs + rl * LD + cv * VO + j);
                v[j] = t.x; v[j + 1] = t.y; v[j + 2] = t.z; v[j + 3] = t.w;
            }
#pragma unroll
            for (int j = 0; j < VO; ++j) v[j] = v[j] * ep.alpha + bias[j];
            if (ep.rowbias) {
#pragma unroll
                for (int j = 0; j < VO; ++j) v[j] += rbv[u][j];
            }
            OutT* o = outb + (long long)row * ep.ldc + col;
            if (fast) {
                if (resb) {
                    if (SAME) {
                        float f[VO];
                        Elem<T>::unpack(resv[u], f);
#pragma unroll
                        for (int j = 0; j < VO; ++j) v[j] += f[j];
                    } else {
#pragma unroll
                        for (int j = 0; j < VO; ++j) v[j] += Elem<T>::ld(resb + (long long)row * ep.res_ld + col + j);
                    }
                }
                if (ep.accumulate) {
                    float f[VO];
                    Elem<OutT>::unpack(accv[u], f);
#pragma unroll
                    for (int j = 0; j < VO; ++j) v[j] += f[j];
                }
                stg16(o, Elem<OutT>::pack(v));
            } else {
#pragma unroll
                for (int j = 0; j < VO; ++j) {
                    if (col + j >= N) break;
                    float x = v[j];
                    if (resb) x += Elem<T>::ld(resb + (long long)row * ep.res_ld + col + j);
                    if (ep.accumulate) x += Elem<OutT>::ld(o + j);
                    Elem<OutT>::st(o + j, x);
                }
            }
        }
    }
    // everything after the first batch (whose load() the caller issued before staging)
    __device__ __forceinline__ void finish_all(const float* cs, const float (&bias)[VO]) {
        finish(0, cs, bias);
        for (int i0 = U; i0 < PER_THREAD; i0 += U) { load(i0); finish(i0, cs, bias); }
    }
};

// element-wise tail for the scatter / atomic output modes (2: fp32 atomic add, 3: NCHW fp32, 4: packed wgrad with atomics,
// 5: packed wgrad, plain stores into the slab copy of this split; a fixed-order sum of the copies (ddpm_wgrad_reduce) then
// gives bit-deterministic gradients.  fp32 atomics run at ~0.33 T elem/s on this chip and plain stores at > 2 T elem/s
// (scripts/probes/atomic_rate.hip), but the atomics stay in L2 while the slabs cost ~33 MB of HBM traffic per layer:
// end to end the two are equally fast)
template <int NT>
__device__ __forceinline__ void epilogue_scatter(const Epilogue& ep, const float* cs, int batch, int row0g, int col0g, int M, int N, int tid,
                                                 int split) {
    // lanes run along n (coalesced atomics for modes 2 / 4); NCHW (mode 3) has N <= a few channels
    for (int idx = tid; idx < TILE * TILE; idx += NT) {
        const int rl = idx >> 7, cl = idx & (TILE - 1);
        const int row = row0g + rl, col = col0g + cl;
        if (row >= M || col >= N) continue;
        float v = cs[rl * CS_LD + cl] * ep.alpha;
        if (ep.bias) v += ep.bias[col];
        if (ep.mode == 2) {
            atomicAdd(reinterpret_cast<float*>(ep.out) + (long long)batch * ep.out_batch_stride + (long long)row * ep.ldc + col, v);
        } else if (ep.mode == 3) {      // row = b*HW + p  ->  out[(b*N + col)*HW + p]
            const unsigned b = fdiv((unsigned)row, ep.dHW);
            const unsigned p = (unsigned)row - b * (unsigned)ep.HW;
            float* o = reinterpret_cast<float*>(ep.out) + ((long long)b * N + col) * ep.HW + p;
            *o = ep.accumulate ? *o + v : v;
        } else {                         // packed weight gradient [n][tap][Creal]; col = tap*Cpad + c
            const unsigned tap = fdiv((unsigned)col, ep.dCpad);
            const int c = col - (int)tap * ep.Cpad;
            if (c < ep.Creal) {
                float* o = reinterpret_cast<float*>(ep.out) + ((long long)row * ep.RS + tap) * ep.Creal + c;
                if (ep.mode == 5) o[(long long)split * ep.slab_stride] = v;
                else if (ep.accumulate) atomicAdd(o, v);
                else *o = v;
            }
        }
    }
}

// One MFMA operand fragment (8 bf16 / 4 fp32 of K per lane) for the 32-row block starting at tile row `rb`, K sub-step kc.
template <typename T, bool TRANS>
__device__ __forceinline__ u32x4 read_frag(const char* tile, int rb, int kc, int lane) {
    if constexpr (TRANS && sizeof(T) == 2) {
        // m-major image (k-rows of 256 bytes): hardware transpose read, two 4-k halves
        const int i16 = lane & 15;
        const int mcol = rb + ((lane >> 4) & 1) * 16 + (i16 & 3) * 4;
        const int krow = kc * 16 + (lane >> 5) * 8 + (i16 >> 2);
        const int pch = (mcol >> 3) ^ (((i16 >> 2) & 3) << 2);
        const char* p = tile + krow * 256 + pch * 16 + (mcol & 7) * 2;
        const uint2 lo = tr_read(p), hi = tr_read(p + 4 * 256);
        u32x4 r;
        r.x = lo.x; r.y = lo.y; r.z = hi.x; r.w = hi.y;
        return r;
    } else {
        // k-contiguous image: row (lane&31), logical 16-byte chunk 2*kc + (lane>>5), swizzle key (row>>1)&7
        const int sw = (lane >> 5) ^ ((lane >> 1) & 7);
        return *reinterpret_cast<const u32x4*>(tile + (rb + (lane & 31)) * ROW_BYTES + (((2 * kc) ^ sw) << 4));
    }
}

#ifdef HALO_TIMING
__device__ unsigned long long* g_halo_timing = nullptr;      // debug builds only: [block][8] = {wall0, clk0, clk_prologue, clk_loop, clk_end, wall_end}
#define HALO_STAMP(slot) do { if (g_halo_timing && threadIdx.x == 0) g_halo_timing[((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 + (slot)] = clock64(); } while (0)
#define HALO_WALL(slot) do { if (g_halo_timing && threadIdx.x == 0) g_halo_timing[((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 + (slot)] = wall_clock64(); } while (0)
#else
#define HALO_STAMP(slot)
#define HALO_WALL(slot)
#endif

// s_waitcnt vmcnt(PER * tiles): allow `tiles` operand-tile pairs (PER LDS-DMA instructions per wave each) to stay in flight
template <int PER>
__device__ __forceinline__ void wait_tiles_in_flight(int tiles) {
    if (tiles >= 3) { if (PER == 8) asm volatile("s_waitcnt vmcnt(24)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(12)" ::: "memory"); }
    else if (tiles == 2) { if (PER == 8) asm volatile("s_waitcnt vmcnt(16)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); }
    else if (tiles == 1) { if (PER == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); }
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// NBUF = 2: classic double buffer, 64 KiB of operand LDS -> two blocks per CU overlap each other's memory latency.
// NBUF = 5 (both operands k-contiguous only): a 5-deep LDS-DMA ring (160 KiB) — four tile pairs are in flight and each step
//           waits with a COUNTED s_waitcnt vmcnt(8 * newer tiles) behind a raw s_barrier.  Used when the grid cannot put
//           two blocks on every CU (small-M layers): one block alone is memory-LATENCY bound per K-step (measured
//           ~0.65 us/step with two tiles in flight), so more tiles in flight is what shortens the step.
// NW = 4: 4 waves as 2(M) x 2(N), 64x64 per wave.  NW = 8: 8 waves as 4(M) x 2(N), 32x64 per wave — twice the waves per CU
//         (two 512-thread blocks) to hide LDS-DMA latency and barrier skew; needs both operands on the DMA path.
// Block order: xcd_logical_id (gfx950.h); the host passes xcd = 1 (g_xcd_swizzle).

#ifndef DEEP_ISSUE_KC
#define DEEP_ISSUE_KC 1
#endif

// SCAT: instantiation for the scatter / atomic output modes only (the weight-gradient products): without the row epilogue's
// prefetch registers the kernel needs fewer VGPRs, which leaves room on the SIMDs for the critical-path kernels that run
// next to it on the other stream.
template <typename T, bool TA, bool TB, int NBUF, int NW, bool SCAT = false>
__global__ __launch_bounds__(NW * 64, NW / 2)
void gemm_kernel(MatDesc A, MatDesc B, Epilogue ep, int M, int N, int K, int k_per_split, int tiles_n, int xcd, FastDiv dtn) {
    HALO_WALL(0); HALO_STAMP(1);
    static_assert(NBUF == 2 || (Loader<T, TA, NW>::DMA && Loader<T, TB, NW>::DMA), "the deep ring needs direct-to-LDS loads on both operands");
    constexpr int NT = NW * 64;
    constexpr int MI = 8 / NW;                              // 32-row accumulator blocks per wave along M
    constexpr int NVEC = 1024 / NT;
    constexpr int VEC = Elem<T>::VEC;
    constexpr int BK = 8 * VEC;
    constexpr int KF = Mma<T>::KF;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int TILE_BYTES = TILE * ROW_BYTES;          // one operand tile; layout: [buf][A | B]
    const int tid = threadIdx.x;
    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;               // wave row block (of 32*MI rows) and column block (of 64)
    const int nsplit = gridDim.y, ntiles = gridDim.x;
    const int lid = xcd_logical_id(blockIdx.x + blockIdx.y * gridDim.x, ntiles * nsplit, xcd);     // tile fastest, then split
    int by = nsplit > 1 ? lid / ntiles : 0, bx = lid - by * ntiles;
    // parity-phase conv (see MatDesc::phase; k-contiguous operands, one split): the tiles of each phase are spread over the 8 XCDs in equal
    // contiguous chunks, heavy phases first — XCD x works on chunk x of every phase, which are the same dy pixels four times (L2 reuse)
    constexpr bool PH_OK = !TA && !TB;
    const bool phase = PH_OK && A.phase;
    if (PH_OK && phase) {
        const int id = blockIdx.x, tp = ntiles >> 2;            // tiles (M x N) per phase
        by = 0; bx = id;
        if (xcd && (tp & 7) == 0) {
            const int tp8 = tp >> 3, j = id >> 3;
            const int p = j / tp8;
            bx = p * tp + (id & 7) * tp8 + (j - p * tp8);
        }
    }
    const int tm = (int)fdiv((unsigned)bx, dtn), tn = bx - tm * tiles_n;
    const int batch = blockIdx.z;
    const int k_begin = by * k_per_split;
    const int k_end = min(K, k_begin + k_per_split);
    if (k_begin >= k_end) return;
    // the tile's non-zero taps, 4 bits each (at most 4 of a 3 x 3 kernel)
    unsigned ph_taps = 0; int ph_ntap = 0;
    if (PH_OK && phase) {
        int a, bb;
        phase_parity(A, (int)fdiv((unsigned)(tm * TILE), A.dMp), a, bb);
        const int py = (a - A.pad_t) & 1, px = (bb - A.pad_l) & 1;
        for (int r = py; r < A.R; r += 2)
            for (int c = px; c < A.S; c += 2) { ph_taps |= (unsigned)(r * A.S + c) << (4 * ph_ntap); ++ph_ntap; }
    }
    // K offset of K-step i of this block
    auto kmap = [&](int i) -> int {
        if (PH_OK && phase) {
            const int ti = (int)fdiv((unsigned)i, A.dSpt);
            return (int)((ph_taps >> (4 * ti)) & 15u) * A.C + (i - ti * A.spt) * BK;
        }
        return k_begin + i * BK;
    };

    Loader<T, TA, NW, 128, PH_OK> la(A, batch, tm * TILE, tid);
    Loader<T, TB, NW, 128, false, TB> lb(B, batch, tn * TILE, tid);      // (k-strided B: the conv view of the weight gradients)

    f32x16 acc[MI][2];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x16)(0.f);

    // bias of this thread's output columns: requested now, consumed in the epilogue (its latency hides under the K loop)
    float bias_v[Elem<T>::VEC];                            // mode 1 (fp32 output, 4 columns per thread) uses the first four
    if constexpr (!SCAT) {
        if (ep.mode == 0) epilogue_bias<T, NT>(ep, tn * TILE, N, tid, bias_v);
        else if (ep.mode == 1) epilogue_bias<float, NT>(ep, tn * TILE, N, tid, *reinterpret_cast<float(*)[4]>(bias_v));
    }

    u32x4 va[NVEC], vb[NVEC];
    constexpr bool DMA_A = Loader<T, TA, NW>::DMA, DMA_B = Loader<T, TB, NW>::DMA;
    auto stage_a = [&](int k0, char* tile) { if constexpr (TA) la.issue_tr(k0, k_end, tile); else la.issue(k0, k_end, tile); };
    auto stage_b = [&](int k0, char* tile) { if constexpr (TB) lb.issue_tr(k0, k_end, tile); else lb.issue(k0, k_end, tile); };
    const int nsteps = (PH_OK && phase) ? ph_ntap * A.spt : (k_end - k_begin + BK - 1) / BK;
    if (nsteps == 0) return;            // (a phase without taps: kernels smaller than the stride; the host does not select the form then)
    // stage the first NBUF-1 K-steps
    if (NBUF == 2) {
        if constexpr (DMA_A) stage_a(kmap(0), smem); else { la.load(k_begin, k_end, va); la.store(smem, va); }
        if constexpr (DMA_B) stage_b(kmap(0), smem + TILE_BYTES); else { lb.load(k_begin, k_end, vb); lb.store(smem + TILE_BYTES, vb); }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    } else {
        if constexpr (DMA_A && DMA_B) {
            // deep ring: NBUF-1 tiles go out before anything is consumed; wait for tile 0 only (counted vmcnt: DMA
            // instructions retire in order, 8 per tile pair)
#pragma unroll
            for (int t = 0; t < NBUF - 1; ++t)
                if (t < nsteps) {
                    stage_a(kmap(t), smem + t * 2 * TILE_BYTES);
                    stage_b(kmap(t), smem + t * 2 * TILE_BYTES + TILE_BYTES);
                }
            wait_tiles_in_flight<32 / NW>(min(NBUF - 2, nsteps - 1));
            __builtin_amdgcn_s_barrier();
        }
    }

    HALO_STAMP(2);
    int cur_i = 0;                                            // ring slot of K-step s
    for (int s = 0; s < nsteps; ++s) {
        const char* cur = smem + cur_i * 2 * TILE_BYTES;
        const int nxt_i = cur_i + 1 == NBUF ? 0 : cur_i + 1;
        char* nxt = smem + nxt_i * 2 * TILE_BYTES;
        const bool more = s + 1 < nsteps;
        if (NBUF == 2) {
            if (more) {       // the other buffer was last read in step s-1: every wave is past that barrier
                const int kn = kmap(s + 1);
                if constexpr (DMA_A) stage_a(kn, nxt); else la.load(kn, k_end, va);
                if constexpr (DMA_B) stage_b(kn, nxt + TILE_BYTES); else lb.load(kn, k_end, vb);
            }
        }
        const char* ta = cur;
        const char* tb = cur + TILE_BYTES;
#pragma unroll
        for (int kc = 0; kc < BK / KF; ++kc) {
            u32x4 fa[MI], fb[2];
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[i] = read_frag<T, TA>(ta, wm * (32 * MI) + i * 32, kc, lane);
#pragma unroll
            for (int j = 0; j < 2; ++j) fb[j] = read_frag<T, TB>(tb, wn * 64 + j * 32, kc, lane);
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) Mma<T>::run(fa[i], fb[j], acc[i][j]);
            if constexpr (NBUF != 2 && DMA_A && DMA_B) {
                // deep ring: the tile NBUF-1 steps ahead is requested in the MIDDLE of the step (its slot — the one of step
                // s-1 — has been free since the last barrier), so the address arithmetic and the LDS-DMA issue overlap
                // the MFMAs already queued instead of delaying the first one
                if (kc == (DEEP_ISSUE_KC < BK / KF ? DEEP_ISSUE_KC : 0) && s + NBUF - 1 < nsteps) {
                    const int far_i = cur_i == 0 ? NBUF - 1 : cur_i - 1;
                    const int kn = kmap(s + NBUF - 1);
                    stage_a(kn, smem + far_i * 2 * TILE_BYTES);
                    stage_b(kn, smem + far_i * 2 * TILE_BYTES + TILE_BYTES);
                }
            }
        }
        if (NBUF == 2) {
            if (more) {
                if constexpr (!DMA_A) la.store(nxt, va);
                if constexpr (!DMA_B) lb.store(nxt + TILE_BYTES, vb);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the LDS-DMA of the next tile has landed
            __syncthreads();
        } else {
            // tile s+1 must have landed; the (up to NBUF-2) tiles issued after it may stay in flight across the barrier
            wait_tiles_in_flight<32 / NW>(min(NBUF - 2, max(nsteps - 2 - s, 0)));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
        cur_i = nxt_i;
    }
    if (NBUF != 2) __syncthreads();     // the epilogue staging below reuses the ring
    HALO_STAMP(3);

    // accumulator (reg r, lane l) -> row (r&3) + 8*(r>>2) + 4*(l>>5), col l&31 of its 32x32 tile; stage as fp32 in LDS.
    float* cs = reinterpret_cast<float*>(smem);
    auto rowmap = [&](int rl) {
        const int row = tm * TILE + rl;
        if (PH_OK && phase) {           // phase-major row -> row of the output tensor
            int ph, b, y, x;
            phase_decode(A, row, ph, b, y, x);
            return (b * A.Ho + y) * A.Wo + x;
        }
        return row < M ? row : -1;
    };
    // accumulators -> fp32 LDS staging (+ the in-launch split-K reduction); false: this block only contributed a slab
    auto stage = [&]() -> bool {
        {
            const int rb = wm * (32 * MI) + 4 * (lane >> 5), cb = wn * 64 + (lane & 31);
            static_for<MI * 32>([&](auto ic) {
                constexpr int idx = decltype(ic)::v;
                constexpr int i = idx >> 5, j = (idx >> 4) & 1, r = idx & 15;
                cs[(rb + i * 32 + (r & 3) + 8 * (r >> 2)) * CS_LD + cb + j * 32] = acc[i][j][r];
            });
        }
        __syncthreads();
        HALO_STAMP(6);
        if (nsplit > 1 && ep.splitk_ws) {
            // In-launch split-K reduction (placement-independent: agent-scope release / acquire around one arrival ticket).
            // Every split publishes its fp32 partial tile as a slab; the LAST arriver adds the other slabs to its own
            // LDS-resident partial and runs the fused epilogue.  Counters return to zero, so no memset between launches.
                    const long long tile_id = (long long)batch * ntiles + bx;
            float* slabs = ep.splitk_ws + tile_id * nsplit * (TILE * TILE);
            float* mine = slabs + (long long)by * (TILE * TILE);
            for (int v = tid; v < TILE * TILE / 4; v += NT) {
                const int r = v >> 5, c4 = (v & 31) << 2;
                *reinterpret_cast<f32x4*>(mine + r * TILE + c4) = *reinterpret_cast<const f32x4*>(cs + r * CS_LD + c4);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            float* flag = cs + TILE;                     // row 0, first padding column: the one shared array holds the flag too
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const unsigned ticket = __hip_atomic_fetch_add(ep.splitk_cnt + tile_id, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                *flag = (ticket == (unsigned)(nsplit - 1)) ? 1.f : 0.f;
            }
            __syncthreads();
            if (*flag == 0.f) return false;
            if (tid == 0) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                __hip_atomic_store(ep.splitk_cnt + tile_id, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            __syncthreads();
            // fixed summation order (slab 0, 1, 2, ...) whichever block happens to arrive last: bit-deterministic results
            for (int v = tid; v < TILE * TILE / 4; v += NT) {
                const int r = v >> 5, c4 = (v & 31) << 2;
                const f32x4 own = *reinterpret_cast<const f32x4*>(cs + r * CS_LD + c4);
                f32x4 a = (by == 0) ? own : *reinterpret_cast<const f32x4*>(slabs + r * TILE + c4);
                for (int sp = 1; sp < nsplit; ++sp) {
                    const f32x4 b = (sp == (int)by) ? own : *reinterpret_cast<const f32x4*>(slabs + (long long)sp * (TILE * TILE) + r * TILE + c4);
                    a.x += b.x; a.y += b.y; a.z += b.z; a.w += b.w;
                }
                *reinterpret_cast<f32x4*>(cs + r * CS_LD + c4) = a;
            }
            __syncthreads();
        }
        return true;
    };
    if constexpr (SCAT) {
        if (!stage()) return;
        epilogue_scatter<NT>(ep, cs, batch, tm * TILE, tn * TILE, M, N, tid, by);
    } else if (ep.mode == 0) {
        RowEpilogue<T, T, NT, TILE, TILE, decltype(rowmap)> re(ep, batch, rowmap, tn * TILE, N, tid);
        re.load(0);
        if (!stage()) return;
        re.finish_all(cs, bias_v);
    } else if (ep.mode == 1) {
        RowEpilogue<T, float, NT, TILE, TILE, decltype(rowmap)> re(ep, batch, rowmap, tn * TILE, N, tid);
        re.load(0);
        if (!stage()) return;
        re.finish_all(cs, *reinterpret_cast<float(*)[4]>(bias_v));
    } else {
        if (!stage()) return;
        epilogue_scatter<NT>(ep, cs, batch, tm * TILE, tn * TILE, M, N, tid, by);
    }
    HALO_STAMP(4); HALO_WALL(5);
}


// =====================================================================================================================
// 64 x 64 tile variant for SMALL grids (the 8x8 / 4x4 levels, 1x1 shortcuts and linears there): with 128x128 tiles those
// layers put 32-128 blocks on 256 CUs and every block is bound by the rate at which ONE CU can move operand tiles into
// LDS (~64 B/clk: 32 KiB per K-step ~ the MFMA time of the step, the two barely overlap).  Quarter-size tiles spread the
// same traffic over 4x the CUs.  k-contiguous operands only (LDS-DMA), 4 waves as 2 x 2 with one 32x32 MFMA block each,
// R-deep ring of 16 KiB stages with counted waits, row epilogue modes 0 / 1.
constexpr int T64 = 64;
constexpr int G64 = 2;            // K-steps per barrier group

// NG = groups in the LDS ring: 3 (96 KiB, one block per CU, two groups in flight) for grids of <= 256 blocks, 2 (64 KiB, two
// blocks per CU, one group in flight) for larger ones where the second resident block hides what the shallower ring exposes.
// EIGHT waves: a wave can only put one LDS-DMA instruction on its way every ~128 clk (scripts/g64_timeline.py: 1024 clk for the
// 8 instructions of a group with 4 waves, against 630 clk for the group's fragment reads + MFMAs, the two strictly one after the
// other with a single wave per SIMD), so the DMA issue is spread over twice the waves and the two waves of a SIMD overlap one's
// DMA issue with the other's math: waves 0-3 take the first K-step of every group, waves 4-7 the second (same 2 x 2 quadrants),
// and the two partial tiles are added through LDS before the epilogue.
template <typename T, int NG>
__global__ __launch_bounds__(512, NG == 2 ? 2 : 1)
void gemm64_kernel(MatDesc A, MatDesc B, Epilogue ep, int M, int N, int K, int tiles_n, int xcd, FastDiv dtn) {
    HALO_WALL(0); HALO_STAMP(1);
    constexpr int BK = 8 * Elem<T>::VEC, KF = Mma<T>::KF, NT = 512;
    static_assert(G64 == 2, "one K-step of a group per wave quartet");
    constexpr int OP_BYTES = T64 * ROW_BYTES;             // one operand tile (8 KiB); stage = [A | B]
    constexpr int GROUP_BYTES = G64 * 2 * OP_BYTES;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kh = wave >> 2, wm = (wave >> 1) & 1, wn = wave & 1;
    const int lid = xcd_logical_id(blockIdx.x, gridDim.x, xcd);
    const int tm = (int)fdiv((unsigned)lid, dtn), tn = lid - tm * tiles_n;
    const int batch = blockIdx.z;
    const int nsplit = gridDim.y, by = blockIdx.y;        // in-launch split-K: each tile's K range in nsplit runs of whole groups
    Loader<T, false, 8, T64> la(A, batch, tm * T64, tid);
    Loader<T, false, 8, T64, false, false> lb(B, batch, tn * T64, tid);
    f32x16 acc0 = (f32x16)(0.f), acc1 = (f32x16)(0.f);   // two accumulators: consecutive MFMAs do not wait on each other
    float bias_t[Elem<T>::VEC], bias_f[4];                // requested now, consumed in the epilogue
    if (ep.mode == 0) epilogue_bias<T, NT, T64>(ep, tn * T64, N, tid, bias_t);
    else epilogue_bias<float, NT, T64>(ep, tn * T64, N, tid, bias_f);
    const int ngroups_all = ((K + BK - 1) / BK + G64 - 1) / G64;
    const int gps = (ngroups_all + nsplit - 1) / nsplit, g0 = by * gps;
    const int ngroups = min(gps, ngroups_all - g0);       // >= 1: the launcher splits only when every run gets groups
    // one group = G64 stages = 4 LDS-DMA instructions per wave (K-steps past the end fetch zeros: out-of-range offsets)
    auto issue_group = [&](int grp, int slot) {
#pragma unroll
        for (int u = 0; u < G64; ++u) {
            la.issue(((g0 + grp) * G64 + u) * BK, K, smem + slot * GROUP_BYTES + u * 2 * OP_BYTES);
            lb.issue(((g0 + grp) * G64 + u) * BK, K, smem + slot * GROUP_BYTES + u * 2 * OP_BYTES + OP_BYTES);
        }
    };
    issue_group(0, 0);
    if (NG > 2 && ngroups > 1) issue_group(1, 1);
    wait_tiles_in_flight<4>(NG > 2 && ngroups > 1 ? 1 : 0);
    __builtin_amdgcn_s_barrier();
    HALO_STAMP(2);
    int slot = 0;
#ifdef HALO_TIMING
    unsigned long long tq0 = 0, tq1 = 0, tq2 = 0, tq3 = 0, tq4 = 0;      // phases of group 8: fragment reads + MFMA issue | DMA issue | vmcnt wait | barrier
#define G64_T(v) do { if (gi == 8) v = clock64(); } while (0)
#else
#define G64_T(v)
#endif
    for (int gi = 0; gi < ngroups; ++gi) {
        const char* base = smem + slot * GROUP_BYTES + kh * 2 * OP_BYTES;
        G64_T(tq0);
        // All fragments of the wave's K-step are requested first, the MFMAs queue on two independent accumulators, then comes
        // the LDS-DMA issue of the group NG-1 ahead (its slot, the one of group gi-1, is free since the last barrier).
        u32x4 fa[BK / KF], fb[BK / KF];
#pragma unroll
        for (int kc = 0; kc < BK / KF; ++kc) {
            fa[kc] = read_frag<T, false>(base, wm * 32, kc, lane);
            fb[kc] = read_frag<T, false>(base + OP_BYTES, wn * 32, kc, lane);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kc = 0; kc < BK / KF; ++kc) {
            if (kc & 1) Mma<T>::run(fa[kc], fb[kc], acc1); else Mma<T>::run(fa[kc], fb[kc], acc0);
        }
        __builtin_amdgcn_sched_barrier(0);
        G64_T(tq1);
        if (gi + NG - 1 < ngroups) issue_group(gi + NG - 1, slot == 0 ? NG - 1 : slot - 1);
        G64_T(tq2);
        wait_tiles_in_flight<4>(NG > 2 && gi + 2 < ngroups ? 1 : 0);   // group gi+1 has landed; group gi+2 may stay in flight
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        G64_T(tq3);
        __builtin_amdgcn_s_barrier();
        G64_T(tq4);
        slot = slot == NG - 1 ? 0 : slot + 1;
    }
    HALO_STAMP(3);
#ifdef HALO_TIMING
    if (g_halo_timing && threadIdx.x == 0)
        g_halo_timing[((blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 8 + 7] =
            ((tq1 - tq0) & 0xffff) | (((tq2 - tq1) & 0xffff) << 16) | (((tq3 - tq2) & 0xffff) << 32) | (((tq4 - tq3) & 0xffff) << 48);
#endif
#undef G64_T
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = acc0[r] + acc1[r];
    // the second K-step's partial tile joins the first's through LDS (the ring is idle: the loop ended on a barrier with no DMA pending)
    float* red = reinterpret_cast<float*>(smem) + (wave & 3) * (16 * 64) + lane;
    if (kh) {
#pragma unroll
        for (int r = 0; r < 16; ++r) red[r * 64] = acc[r];
    }
    // epilogue: fp32 staging [64][68]
    constexpr int LD64 = T64 + 4;
    float* cs = reinterpret_cast<float*>(smem);
    auto rowmap = [&](int rl) { const int row = tm * T64 + rl; return row < M ? row : -1; };
    RowEpilogue<T, T, NT, T64, T64, decltype(rowmap)> re_t(ep, batch, rowmap, tn * T64, N, tid);
    RowEpilogue<T, float, NT, T64, T64, decltype(rowmap)> re_f(ep, batch, rowmap, tn * T64, N, tid);
    if (ep.mode == 0) re_t.load(0); else re_f.load(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (!kh) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] += red[r * 64];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();              // every partial has been read before the staging overwrites it
    if (!kh) {
        const int rb = wm * 32 + 4 * (lane >> 5), cb = wn * 32 + (lane & 31);
        static_for<16>([&](auto ic) {
            constexpr int r = decltype(ic)::v;
            cs[(rb + (r & 3) + 8 * (r >> 2)) * LD64 + cb] = acc[r];
        });
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    HALO_STAMP(6);
    if (nsplit > 1) {
        // Every run publishes its fp32 partial tile as a slab, takes an arrival ticket, and the LAST arriver adds the slabs in run
        // order (bit-deterministic whoever arrives last) and carries on into the epilogue; the counter goes back to zero (no memset
        // between launches).  The slabs move with agent-scope (write-through / L2-bypassing) accesses, dword by dword, instead of
        // plain stores bracketed by release / acquire fences: a fence writes back and invalidates the XCD's whole L2 — 5 us here,
        // more with a step's worth of dirty activations in it.
        const long long tile_id = (long long)batch * gridDim.x + lid;
        float* slabs = ep.splitk_ws + tile_id * nsplit * (T64 * T64);
        float* mine = slabs + (long long)by * (T64 * T64);
        // 16-byte agent-scope accesses (global_* ... sc1), two per thread and slab: thread q owns elements 4 q .. 4 q + 3 of the tile
        f32x4 own[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int q = tid + NT * h;
            own[h] = *reinterpret_cast<const f32x4*>(cs + (q >> 4) * LD64 + (q & 15) * 4);
            asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(mine + q * 4), "v"(own[h]) : "memory");
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        float* flag = cs + T64;                      // row 0, first padding column
        if (tid == 0) {
            const unsigned ticket = __hip_atomic_fetch_add(ep.splitk_cnt + tile_id, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *flag = (ticket == (unsigned)(nsplit - 1)) ? 1.f : 0.f;
            if (ticket == (unsigned)(nsplit - 1)) __hip_atomic_store(ep.splitk_cnt + tile_id, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        __syncthreads();
        if (*flag == 0.f) return;
        // all the other runs' vectors are requested before the first is used (up to 7 x 2 loads in flight), then added in run order
        // (buffer loads with the sc1 cache-policy bit, not inline asm: the compiler tracks their destination registers and places the
        //  waits itself — an asm load whose wait sits in a separate asm statement leaves the register allocator free to move or spill
        //  the destination before the data has landed)
        constexpr int MAXR = 8;
        f32x4 other[MAXR][2];
        const __amdgpu_buffer_rsrc_t slab_rs = __builtin_amdgcn_make_buffer_rsrc(slabs, 0, nsplit * (T64 * T64) * 4, 0x00020000);
#pragma unroll
        for (int sp = 0; sp < MAXR; ++sp) {
            if (sp < nsplit && sp != by) {
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    other[sp][h] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(slab_rs, (sp * (T64 * T64) + (tid + NT * h) * 4) * 4, 0, 16));
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 a4 = (f32x4)(0.f);
#pragma unroll
            for (int sp = 0; sp < MAXR; ++sp)
                if (sp < nsplit) a4 += (sp == by) ? own[h] : other[sp][h];
            const int q = tid + NT * h;
            *reinterpret_cast<f32x4*>(cs + (q >> 4) * LD64 + (q & 15) * 4) = a4;
        }
        __syncthreads();
    }
    if (ep.mode == 0) re_t.finish_all(cs, bias_t);
    else re_f.finish_all(cs, bias_f);
    HALO_STAMP(4); HALO_WALL(5);
}
template __global__ void gemm64_kernel<bf16_t, 2>(MatDesc, MatDesc, Epilogue, int, int, int, int, int, FastDiv);
template __global__ void gemm64_kernel<bf16_t, 3>(MatDesc, MatDesc, Epilogue, int, int, int, int, int, FastDiv);
template __global__ void gemm64_kernel<float, 2>(MatDesc, MatDesc, Epilogue, int, int, int, int, int, FastDiv);
template __global__ void gemm64_kernel<float, 3>(MatDesc, MatDesc, Epilogue, int, int, int, int, int, FastDiv);

// =====================================================================================================================
// 3x3 / stride 1 / pad 1 convolution with a STATIONARY INPUT HALO (bf16): the hot conv of the UNet (forward and dgrad).
//
// The generic implicit GEMM re-fetches every input pixel 9x (once per tap) and every weight tile once per 128 pixels;
// at ~30 % MFMA utilisation its L2 -> LDS stream (TCC_BUSY 75 %) is the limiter.  Here a block owns 256 output pixels
// (NB images x PH x PW patch, e.g. one 16x16 patch) x 128 output channels and walks K as (64-channel chunk, tap):
//   * the input halo of the patch ((PH+2) x (PW+2) pixels x 64 channels, zero-padded by out-of-range buffer offsets) is
//     DMA'd to LDS ONCE per chunk and serves all 9 taps — the A fragment of tap (r,s) is the same LDS tile read at pixel
//     offset r*(PW+2)+s;
//   * only the 128 x 64 weight tile streams per tap (double-buffered LDS-DMA), shared by twice as many pixels as before.
// L2 -> LDS bytes per FLOP drop to ~1/3 of the generic kernel's.  8 waves as 4(M) x 2(N), 64x64 per wave; one block per CU.
struct Conv3Args {
    const void* x; long long x_ld; unsigned x_extent;
    const void* w; unsigned w_extent;
    int B, H, W, C, N, K;
    int PH, PW, NB, lPW, lPP;         // patch geometry: PW and PH*PW are powers of two (log2 in lPW, lPP); NB*PH*PW == 256
    int ky;                           // 1 when the halo row parity takes part in the LDS swizzle key (8-wide patches)
    int tiles_y, tiles_x;             // patches per image
    FastDiv d_tiles_n, d_tpi, d_tiles_x, d_halo_img, d_halo_w;     // host-prepared divisors: no runtime integer division in the prologue
    Epilogue ep;
};
constexpr int C3_NI = 7;              // halo DMA parts of 512 vectors: up to 448 halo pixels x 8 chunks

// RING = depth of the weight-tile ring (RING-1 tiles in flight, counted s_waitcnt + raw s_barrier); HROWS = LDS rows
// reserved per halo buffer.  LDS = 2*HROWS*128 + RING*16 KiB = 160 KiB in both instantiated configurations.
template <int RING, int HROWS>
__global__ __launch_bounds__(512, 2)
void conv3x3_halo_kernel(Conv3Args a, int tiles_n, int xcd) {
    HALO_WALL(0); HALO_STAMP(1);
    typedef bf16_t T;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // LDS: [halo 0 | halo 1 | weight ring]; the fp32 epilogue staging (64 rows) aliases the halo region afterwards
    constexpr int HALO_BYTES = HROWS * ROW_BYTES, BT_BYTES = TILE * ROW_BYTES;
    char* halo = smem;
    char* btile = smem + 2 * HALO_BYTES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave >> 1, wn = wave & 1;
    const int lid = xcd_logical_id(blockIdx.x, gridDim.x, xcd);
    const int tmi = (int)fdiv((unsigned)lid, a.d_tiles_n), tn = lid - tmi * tiles_n;
    const int tpi = a.tiles_y * a.tiles_x;
    const int grp = (int)fdiv((unsigned)tmi, a.d_tpi), pt = tmi - grp * tpi;
    const int ty = (int)fdiv((unsigned)pt, a.d_tiles_x), tx = pt - ty * a.tiles_x;
    const int py0 = ty * a.PH, px0 = tx * a.PW, img0 = grp * a.NB;
    const int HH = a.PH + 2, HWd = a.PW + 2, HP = a.NB * HH * HWd;
    const int ES = 2;

    const __amdgpu_buffer_rsrc_t rx = buffer_rsrc(a.x, a.x_extent), rw = buffer_rsrc(a.w, a.w_extent);

    // LDS swizzle of the halo rows (128 B each, bank half = hp & 1 = hx & 1 since the halo pitch is even): the 16-byte
    // chunk c of halo pixel (hy, hx) sits at physical chunk c ^ key, key = (hx >> 1) ^ ((hy & ky) << 2).  With it the 16
    // pixels one ds_read_b128 lane group touches (two half patch rows, or four quarter rows of an 8-wide patch) land on
    // 16 distinct (bank half, chunk) pairs for every tap shift — the address-derived key (hp >> 1) was 2-3 way conflicted.
    // halo DMA plan: vector v = tid + 512 i -> halo pixel hp = v>>3, physical chunk v&7 (logical chunk ^ key)
    unsigned hoff[C3_NI];
#pragma unroll
    for (int i = 0; i < C3_NI; ++i) {
        const int v = tid + 512 * i, hp = v >> 3;
        const int img = (int)fdiv((unsigned)hp, a.d_halo_img), rem = hp - img * (HH * HWd);
        const int hy = (int)fdiv((unsigned)rem, a.d_halo_w), hx = rem - hy * HWd;
        const int iy = py0 + hy - 1, ix = px0 + hx - 1, gi = img0 + img;
        const bool ok = hp < HP && gi < a.B && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W;
        const int lc = (v & 7) ^ (((hx >> 1) ^ ((hy & a.ky) << 2)) & 7);
        hoff[i] = ok ? (unsigned)((((long long)(gi * a.H + iy) * a.W + ix) * a.x_ld + lc * 8) * ES) : BUF_OOB;
    }
    // weight DMA plan: vector v = tid + 512 i -> row n = v>>3 of the 128-row tile, physical chunk v&7
    unsigned woff[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int v = tid + 512 * i, row = v >> 3, n = tn * TILE + row;
        const int lc = (v & 7) ^ ((row >> 1) & 7);
        woff[i] = n < a.N ? (unsigned)(((long long)n * a.K + lc * 8) * ES) : BUF_OOB;
    }
    auto issue_halo_part = [&](unsigned ho, int i, int cc, char* dst) {     // part i of the halo of channel chunk cc
        const unsigned o = ho == BUF_OOB ? BUF_OOB : ho + (unsigned)(cc * 64 * ES);
        LDS_DMA16(rx, dst + (wave * 64 + 512 * i) * 16, o, 0);
    };
    const int nchunks = a.C / 64;
    const int total = nchunks * 9;                        // K-steps: (channel chunk, tap)
    auto issue_w = [&](int step) {                          // weight tile of K-step `step` into its ring slot
        const int cc = step / 9, tap = step - 9 * cc;
        char* dst = btile + (step % RING) * BT_BYTES;
        const unsigned koff = (unsigned)((tap * a.C + cc * 64) * ES);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const unsigned o = woff[i] == BUF_OOB ? BUF_OOB : woff[i] + koff;
            LDS_DMA16(rw, dst + (wave * 64 + 512 * i) * 16, o, 0);
        }
    };

    // this lane's output pixels (rows of its two 32-row accumulator blocks) -> halo index of tap (0,0)
    int hp0[2], pxl[2], pyl[2];
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
        const int p = wm * 64 + mi * 32 + (lane & 31);
        const int il = p >> a.lPP, q = p & ((1 << a.lPP) - 1);
        const int py = q >> a.lPW, px = q & (a.PW - 1);
        hp0[mi] = il * HH * HWd + py * HWd + px;
        pxl[mi] = px; pyl[mi] = py & a.ky;
    }

    f32x16 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (f32x16)(0.f);
    float bias[8];                                        // requested now, consumed in the epilogue
    epilogue_bias<T, 512>(a.ep, tn * TILE, a.N, tid, bias);

    const int ni = (HP * 8 + 511) / 512;                 // halo DMA parts actually needed
    // prologue: halo of chunk 0, then the first RING-1 weight tiles; wait for halo + tile 0 only
#pragma unroll
    for (int i = 0; i < C3_NI; ++i)
        if (i < ni) issue_halo_part(hoff[i], i, 0, halo);
#pragma unroll
    for (int t = 0; t < RING - 1; ++t)
        if (t < total) issue_w(t);
    if (total >= RING - 1) { if (RING == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory"); else asm volatile("s_waitcnt vmcnt(2)" ::: "memory"); }
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    HALO_STAMP(2);

    const int hi = lane >> 5;
    int step = 0;
    for (int cc = 0; cc < nchunks; ++cc) {
        const char* hcur = halo + (cc & 1) * HALO_BYTES;
        char* hnxt = halo + ((cc + 1) & 1) * HALO_BYTES;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap, ++step) {     // fully unrolled: the halo-part index must be a constant
            const char* bcur = btile + (step % RING) * BT_BYTES;
            // in program order: next chunk's halo part first, then the weight tile RING-1 steps ahead (its slot was read
            // in step-1; every wave is past that barrier).  Loads retire in order, so once tile (cc+1, 0) has landed the
            // whole next halo has too.
            if (tap < C3_NI && tap < ni && cc + 1 < nchunks) issue_halo_part(hoff[tap < C3_NI ? tap : 0], tap, cc + 1, hnxt);
            if (step + RING - 1 < total) issue_w(step + RING - 1);
            const int r = tap / 3, s = tap - 3 * r;
            const int shift = r * HWd + s;
#pragma unroll
            for (int kc = 0; kc < 4; ++kc) {
                u32x4 fa[2], fb[2];
#pragma unroll
                for (int mi = 0; mi < 2; ++mi) {
                    const int hp = hp0[mi] + shift;
                    const int key = (((pxl[mi] + s) >> 1) ^ (((pyl[mi] + r) & a.ky) << 2)) & 7;
                    fa[mi] = *reinterpret_cast<const u32x4*>(hcur + hp * ROW_BYTES + ((((2 * kc) | hi) ^ key) << 4));
                }
#pragma unroll
                for (int j = 0; j < 2; ++j) fb[j] = read_frag<T, false>(bcur, wn * 64 + j * 32, kc, lane);
#pragma unroll
                for (int mi = 0; mi < 2; ++mi)
#pragma unroll
                    for (int j = 0; j < 2; ++j) Mma<T>::run(fa[mi], fb[j], acc[mi][j]);
            }
            // tile step+1 must have landed; the RING-2 newer tiles (2 DMA instructions each) may stay in flight
            const int newer = total - 2 - step;         // tiles issued after tile step+1
            if (RING == 4 && newer >= 2) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
            else if (newer >= 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
        }
    }
    __syncthreads();
    HALO_STAMP(3);

    // epilogue: the whole 256 x 128 fp32 tile is staged at once (132 KiB of the now idle LDS) — one barrier, then every
    // thread streams 16-byte vectors out; nothing waits for the stores to be acknowledged.
    float* cs = reinterpret_cast<float*>(smem);
    auto rowmap = [&](int p) {
        const int il = p >> a.lPP, qq = p & ((1 << a.lPP) - 1);
        const int gi = img0 + il;
        return gi < a.B ? (gi * a.H + py0 + (qq >> a.lPW)) * a.W + px0 + (qq & (a.PW - 1)) : -1;
    };
    RowEpilogue<T, T, 512, 256, TILE, decltype(rowmap)> re(a.ep, 0, rowmap, tn * TILE, a.N, tid);
    re.load(0);
    {
        const int rb = wm * 64 + 4 * (lane >> 5), cb = wn * 64 + (lane & 31);
        static_for<64>([&](auto ic) {
            constexpr int idx = decltype(ic)::v;
            constexpr int i = idx >> 5, j = (idx >> 4) & 1, rr = idx & 15;
            cs[(rb + i * 32 + (rr & 3) + 8 * (rr >> 2)) * CS_LD + cb + j * 32] = acc[i][j][rr];
        });
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    HALO_STAMP(6);
    re.finish_all(cs, bias);
    HALO_STAMP(4); HALO_WALL(5);
}

#ifdef HALO_TIMING
extern "C" int ddpm_debug_set_halo_timing(void* p) {
    return hipMemcpyToSymbol(HIP_SYMBOL(g_halo_timing), &p, sizeof(p)) == hipSuccess ? 0 : -1;
}
#endif

// Explicit instantiations: every (dtype, operand layout, ring depth, wave count) the launcher can pick.
#define INST(T, TA, TB, NB, NWV) template __global__ void gemm_kernel<T, TA, TB, NB, NWV>(MatDesc, MatDesc, Epilogue, int, int, int, int, int, int, FastDiv);
INST(bf16_t, false, false, 2, 8) INST(bf16_t, false, false, 5, 8)
INST(bf16_t, false, true, 2, 8) INST(bf16_t, true, false, 2, 8) INST(bf16_t, true, true, 2, 8)
INST(float, false, false, 2, 8) INST(float, false, false, 5, 8)
INST(float, false, true, 2, 4) INST(float, true, false, 2, 4) INST(float, true, true, 2, 4)
#undef INST
template __global__ void gemm_kernel<bf16_t, true, true, 2, 8, true>(MatDesc, MatDesc, Epilogue, int, int, int, int, int, int, FastDiv);

// =====================================================================================================================
// Fused single-head attention forward (inference): O = softmax(Q K^T * scale) V for one image per blockIdx.y, 128 queries
// per block (4 waves x 32 queries), keys / values streamed in chunks of 64 through LDS; the L x L logits never leave the
// chip.  Reference: AttentionBlock.forward, ddpm_torch/models/unet.py:41-52.
//
// Formulated TRANSPOSED so that no operand ever has to be re-laid-out through LDS:
//   S^T[key, q] = K Q^T      A = K chunk (rows = keys), B = Q tile (rows = queries), both k-contiguous LDS-DMA tiles;
//   a lane of the 32x32 accumulator owns ONE query (column lane&31) and 16 keys per block -> the softmax over keys is a
//   per-lane register reduction plus one exchange between the two half-waves (online max / sum across chunks);
//   O^T[dv, q] += V^T P^T    B = P^T straight from the S^T accumulator registers (the contraction index is the key, so
//   the MFMA k-slots simply follow the accumulator's key order 16t + 4g + {0..3}, 16t + 8 + 4g + {0..3}); A = V^T read
//   from the V chunk AS STORED (key-major) with the hardware transpose read in the same key order.
template <int DB>          // head dimension D = 32 * DB (DB = 4 or 8)
__global__ __launch_bounds__(256)
void attn_fwd_kernel(MatDesc Qd, MatDesc Kd, MatDesc Vd, bf16_t* __restrict__ out, long long out_ld, int L, float scale) {
    typedef bf16_t T;
    constexpr int D = 32 * DB, DC = D / 64, VT = D / 128;
    constexpr int Q_BYTES = TILE * ROW_BYTES, K_BYTES = 64 * ROW_BYTES, V_BYTES = 64 * 256;
    constexpr int NK = 2 * DC, NV_ = 4 * VT;                  // LDS-DMA instructions per thread: one K chunk / one V chunk
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qs = smem;                                          // [DC][128 q][64 d]
    char* Ks = Qs + DC * Q_BYTES;                             // [DC][64 keys][64 d]
    char* Vs = Ks + DC * K_BYTES;                             // [VT][64 keys][128 dv] (key-major image)
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 5;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.y, q0 = blockIdx.x * TILE;
    const int nchunks = L / 64;

    auto wait_vm = [&](int n) {                               // n in {0, 4, 8}
        if (n == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
        else if (n == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    };
    Loader<T, true, 4> lv0(Vd, b, 0, tid), lv1(Vd, b, VT > 1 ? 128 : 0, tid);
    auto issue_k = [&](int chunk) {
        Loader<T, false, 4, 64> lk(Kd, b, chunk * 64, tid);
#pragma unroll
        for (int c = 0; c < DC; ++c) lk.issue(c * 64, D, Ks + c * K_BYTES);
    };
    auto issue_v = [&](int chunk) {
        lv0.issue_tr(chunk * 64, L, Vs);
        if (VT > 1) lv1.issue_tr(chunk * 64, L, Vs + V_BYTES);
    };
    {
        Loader<T, false, 4, 128> lq(Qd, b, q0, tid);
#pragma unroll
        for (int c = 0; c < DC; ++c) lq.issue(c * 64, D, Qs + c * Q_BYTES);
    }
    issue_k(0);
    issue_v(0);

    f32x16 acc_o[DB];
#pragma unroll
    for (int j = 0; j < DB; ++j) acc_o[j] = (f32x16)(0.f);
    float m_run = -3.0e38f, l_run = 0.f;                      // running max (scaled logits) and sum for this lane's query

    for (int ch = 0; ch < nchunks; ++ch) {
        wait_vm(NV_);                                         // Q and this K chunk have landed; the V chunk may still fly
        __builtin_amdgcn_s_barrier();
        // ---- S^T = K Q^T for 64 keys x this wave's 32 queries
        f32x16 acc_s[2] = {(f32x16)(0.f), (f32x16)(0.f)};
#pragma unroll
        for (int c = 0; c < DC; ++c)
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const u32x4 fq = read_frag<T, false>(Qs + c * Q_BYTES, wave * 32, kk, lane);
#pragma unroll
                for (int i = 0; i < 2; ++i) {
                    const u32x4 fk = read_frag<T, false>(Ks + c * K_BYTES, i * 32, kk, lane);
                    Mma<T>::run(fk, fq, acc_s[i]);
                }
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // every wave is done with the K chunk
        if (ch + 1 < nchunks) issue_k(ch + 1);
        // ---- online softmax over the keys of this chunk (per lane: one query)
        float mloc = acc_s[0][0];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) mloc = fmaxf(mloc, acc_s[i][r]);
        mloc = fmaxf(mloc, __shfl_xor(mloc, 32, 64));
        const float m_new = fmaxf(m_run, mloc * scale);
        const float alpha = __expf(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
        u32x4 pb[2][2];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float e[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) { e[r] = __expf(acc_s[i][8 * t + r] * scale - m_new); psum += e[r]; }
                pb[i][t] = u32x4{pack_bf2(e[0], e[1]), pack_bf2(e[2], e[3]), pack_bf2(e[4], e[5]), pack_bf2(e[6], e[7])};
            }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int j = 0; j < DB; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc_o[j][r] *= alpha;
        // ---- O^T += V^T P^T
        wait_vm(ch + 1 < nchunks ? NK : 0);                   // this V chunk has landed (the next K chunk may still fly)
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int kb = i * 32 + t * 16;
#pragma unroll
                for (int j = 0; j < DB; ++j) {
                    // V^T fragment of dv block j in the accumulator's key order: keys kb + 4g + {0..3}, kb + 8 + 4g + {0..3}
                    const int i16 = lane & 15;
                    const int mcol = (j & 3) * 32 + ((lane >> 4) & 1) * 16 + (i16 & 3) * 4;
                    const int krow = kb + g * 4 + (i16 >> 2);
                    const int pch = (mcol >> 3) ^ (((i16 >> 2) & 3) << 2);
                    const char* p = Vs + (j >> 2) * V_BYTES + krow * 256 + pch * 16 + (mcol & 7) * 2;
                    const uint2 lo = tr_read(p), hi = tr_read(p + 8 * 256);
                    u32x4 fv;
                    fv.x = lo.x; fv.y = lo.y; fv.z = hi.x; fv.w = hi.y;
                    Mma<T>::run(fv, pb[i][t], acc_o[j]);
                }
            }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();                         // every wave is done with the V chunk
        if (ch + 1 < nchunks) issue_v(ch + 1);
    }
    // ---- normalise and store: this lane owns query q, and per accumulator register quad 4 consecutive channels
    const float l_tot = l_run + __shfl_xor(l_run, 32, 64);
    const float inv = 1.0f / l_tot;
    const int q = q0 + wave * 32 + (lane & 31);
    T* orow = out + ((long long)b * L + q) * out_ld;
#pragma unroll
    for (int j = 0; j < DB; ++j)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
            uint2 w;
            w.x = pack_bf2(acc_o[j][4 * rq] * inv, acc_o[j][4 * rq + 1] * inv);
            w.y = pack_bf2(acc_o[j][4 * rq + 2] * inv, acc_o[j][4 * rq + 3] * inv);
            *reinterpret_cast<uint2*>(orow + j * 32 + 8 * rq + 4 * g) = w;
        }
}
template __global__ void attn_fwd_kernel<4>(MatDesc, MatDesc, MatDesc, bf16_t*, long long, int, float);
template __global__ void attn_fwd_kernel<8>(MatDesc, MatDesc, MatDesc, bf16_t*, long long, int, float);

// ---------------------------------------------------------------------------------------------- host side

// Kernel ids reported by the ddpm_*_variant queries (bench.py attributes its per-launch timings with them):
// 1 gemm_kernel 4-wave, 2 gemm_kernel 8-wave, 3 gemm_kernel deep ring, 4 gemm64_kernel, 5 conv3x3_halo_kernel, 7 pw_conv_kernel (pointwise.hip), 8 / 10 conv3x3_stream_kernel (conv3x3.hip, 16 x 16 / 8 x 8 patches), 13 conv3x3_pc_kernel (conv3x3.hip, loader / consumer waves), 11 / 12 conv3x3_few_out / few_in (edgeconv.hip).
// The queries run the SAME dispatch code with `dry` set (nothing is launched): the library keeps no mutable state.
static constexpr int g_xcd_swizzle = 1;      // the kernels' `xcd` argument: XCD-aware block order (see xcd_logical_id), always on
static thread_local int g_variant_query = 0, g_variant_result = 0;      // scoped to ONE ddpm_*_variant call (set and cleared inside it)

struct GemmArgs {          // plain-C mirror filled by the extern "C" entry points
    MatDesc A, B;
    Epilogue ep;
    int M, N, K, batch, splits, dtype;
    int dry, variant;      // dry: decide the kernel (-> variant) but launch nothing
};

static int conv3x3_halo_launch(GemmArgs& g, const void* x, long long x_ld, const void* w, int B, int H, int W, int C, int N, hipStream_t st) {
    // patch geometry: 256 output pixels per block
    int PW = W >= 16 ? 16 : W, PH = H >= 16 ? 16 : H;
    while (PH * PW > 256) PH >>= 1;
    const int NB = 256 / (PH * PW);
    auto ilog2 = [](int v) { int l = 0; while ((1 << l) < v) ++l; return l; };
    if ((PW & (PW - 1)) || ((PH * PW) & (PH * PW - 1)) || H % PH || W % PW || NB * PH * PW != 256) return -1;
    const int HP = NB * (PH + 2) * (PW + 2);
    if (HP > 448) return -1;
    Conv3Args a;
    memset(&a, 0, sizeof(a));
    a.x = x; a.x_ld = x_ld; a.w = w;
    a.B = B; a.H = H; a.W = W; a.C = C; a.N = N; a.K = 9 * C;
    const long long xbytes = ((long long)B * H * W * x_ld - (x_ld - C)) * 2, wbytes = (long long)N * 9 * C * 2;
    if (xbytes > BUF_OOB || wbytes > BUF_OOB) return -1;
    a.x_extent = (unsigned)xbytes; a.w_extent = (unsigned)wbytes;
    a.PH = PH; a.PW = PW; a.NB = NB; a.lPW = ilog2(PW); a.lPP = ilog2(PH * PW);
    a.ky = PW == 8 ? 1 : 0;
    a.tiles_y = H / PH; a.tiles_x = W / PW;
    a.d_tiles_n = make_fastdiv((unsigned)((N + TILE - 1) / TILE)); a.d_tpi = make_fastdiv((unsigned)(a.tiles_y * a.tiles_x));
    a.d_tiles_x = make_fastdiv((unsigned)a.tiles_x);
    a.d_halo_img = make_fastdiv((unsigned)((PH + 2) * (PW + 2))); a.d_halo_w = make_fastdiv((unsigned)(PW + 2));
    a.ep = g.ep;
    const int groups = (B + NB - 1) / NB, tiles_n = (N + TILE - 1) / TILE;
    const dim3 grid(groups * a.tiles_y * a.tiles_x * tiles_n);
    constexpr int LDS = 160 * 1024;                       // both configurations fill the CU's LDS
#define C3_LAUNCH(RING, HROWS)                                                                                          \
    do {                                                                                                                 \
        static DevOnce attr_set;                                                                                    \
        if (!attr_set) {                                                                                                 \
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&conv3x3_halo_kernel<RING, HROWS>),                    \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, LDS) != hipSuccess) return DDPM_ERR_LAUNCH; \
            attr_set = true;                                                                                             \
        }                                                                                                                \
        hipLaunchKernelGGL((conv3x3_halo_kernel<RING, HROWS>), grid, dim3(512), LDS, st, a, tiles_n, g_xcd_swizzle);                    \
    } while (0)
    g.variant = 5;
    if (g.dry) return DDPM_OK;
    if (HP <= 384) C3_LAUNCH(4, 384);      // one 16x16 patch: 2 x 48 KiB halo + 4 x 16 KiB weight ring
    else C3_LAUNCH(3, 448);                // four 8x8 patches: 2 x 56 KiB halo + 3 x 16 KiB weight ring
#undef C3_LAUNCH
    return check_launch();
}

static int finish_desc(MatDesc& d, int esize) {
    // extent of the region one batch of the operand can touch (the buffer descriptor's num_records)
    const long long elems = d.conv ? (long long)d.conv_batches * d.H * d.W * d.ld - (d.ld - d.C)
                                   : (long long)(d.n_slow - 1) * d.ld + d.n_fast;
    const long long bytes = elems * esize;
    if (bytes <= 0 || bytes > BUF_OOB) return DDPM_ERR_SHAPE;      // 32-bit buffer offsets: operands < 2 GiB
    d.extent_bytes = (unsigned)bytes;
    if (d.conv) {
        d.dHoWo = make_fastdiv((unsigned)(d.Ho * d.Wo));
        d.dWo = make_fastdiv((unsigned)d.Wo);
        d.dC = make_fastdiv((unsigned)d.C);
        d.dS = make_fastdiv((unsigned)d.S);
    }
    return DDPM_OK;
}

template <typename T>
static int launch_t(GemmArgs& g, hipStream_t st) {
    constexpr int BK = 8 * Elem<T>::VEC;
    const int tiles_m = (g.M + TILE - 1) / TILE, tiles_n = (g.N + TILE - 1) / TILE;
    int splits = g.splits < 1 ? 1 : g.splits;
    int ksteps = (g.K + BK - 1) / BK;
    int steps_per = (ksteps + splits - 1) / splits;
    splits = (ksteps + steps_per - 1) / steps_per;
    if (splits > 1 && g.ep.mode != 2 && g.ep.mode != 4 && g.ep.mode != 5 && !(g.ep.splitk_ws && g.ep.splitk_cnt)) return DDPM_ERR_SHAPE;
    if (g.ep.mode == 5 && splits != g.splits) return DDPM_ERR_SHAPE;      // every slab copy the caller will sum must be written
    if (g.ep.mode == 2 || g.ep.mode == 4 || g.ep.mode == 5) { g.ep.splitk_ws = nullptr; g.ep.splitk_cnt = nullptr; }
    dim3 grid(tiles_m * tiles_n, splits, g.batch);
    // small grids of k-contiguous products: 64x64 tiles put 4x as many CUs to work (see gemm64_kernel)
    constexpr int t64_max_tiles = 64;
    if (!g.A.phase && !g.A.trans && !g.B.trans && (splits == 1 || (splits == 2 && g.ep.splitk_ws && g.ep.splitk_cnt)) &&
        (g.ep.mode == 0 || g.ep.mode == 1) && (long long)tiles_m * tiles_n * g.batch <= t64_max_tiles) {
        const int t64n = (g.N + T64 - 1) / T64;
        // two K runs per tile when the caller offers the workspace (splits == 2), the tiles alone leave half the CUs idle and every
        // run still gets >= 4 groups: the loop is bound by what ONE CU can move into its LDS (scripts/g64_timeline.py)
        const int groups64 = ((g.K + BK - 1) / BK + G64 - 1) / G64;
        // (round 3) up to eight runs where the tiles are fewer still — the 16 x 16 / 8 x 8 levels at the CelebA-HQ per-GPU batch of 2 have
        // 16-64 tiles and K = 2304 / 4608: as long as tiles x runs <= 256 and a run keeps >= 4 groups
        int sp64 = 1;
        if (splits == 2) {
            const long long tiles64 = (long long)((g.M + T64 - 1) / T64) * t64n * g.batch;
            constexpr int max_runs = 8;
            while (sp64 * 2 <= max_runs && tiles64 * sp64 * 2 <= 256 && groups64 / (sp64 * 2) >= 4) sp64 *= 2;
        }
        const dim3 grid64(((g.M + T64 - 1) / T64) * t64n, sp64, g.batch);
#define LAUNCH64(NG)                                                                                                     \
    do {                                                                                                                 \
        constexpr int LDS64 = NG * G64 * 2 * T64 * ROW_BYTES;                                                            \
        static DevOnce attr_set;                                                                                    \
        if (!attr_set) {                                                                                                 \
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm64_kernel<T, NG>), hipFuncAttributeMaxDynamicSharedMemorySize, LDS64) != hipSuccess) \
                return DDPM_ERR_LAUNCH;                                                                                  \
            attr_set = true;                                                                                             \
        }                                                                                                                \
        hipLaunchKernelGGL((gemm64_kernel<T, NG>), grid64, dim3(512), LDS64, st, g.A, g.B, g.ep, g.M, g.N, g.K, t64n, g_xcd_swizzle, make_fastdiv((unsigned)t64n));   \
    } while (0)
        g.variant = 4;
        if (g.dry) return DDPM_OK;
        if ((long long)grid64.x * grid64.y * grid64.z <= 256) LAUNCH64(3); else LAUNCH64(2);
#undef LAUNCH64
        return check_launch();
    }
    const size_t lds2 = TILE * CS_LD * sizeof(float);     // 4 operand tiles (64 KiB) <= fp32 epilogue staging (66 KiB)
    const size_t lds3 = 10 * TILE * ROW_BYTES;            // 5-deep ring: 160 KiB, one block per CU
    const int kps = steps_per * BK;
    // deep ring when the grid cannot keep two blocks on each of the 256 CUs anyway
    const bool deep = !g.A.trans && !g.B.trans && (long long)grid.x * grid.y * grid.z <= 256 && steps_per >= 3;

#define LAUNCH(TA, TB, NB, NWV, LDS)                                                                                     \
    do {                                                                                                                 \
        g.variant = NB != 2 ? 3 : (NWV == 8 ? 2 : 1);                                                                    \
        if (g.dry) break;                                                                                                \
        static DevOnce attr_set;   /* > 64 KiB of dynamic LDS needs the opt-in once per instantiation */            \
        if (!attr_set) {                                                                                                 \
            if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_kernel<T, TA, TB, NB, NWV>),                     \
                                    hipFuncAttributeMaxDynamicSharedMemorySize, (int)(LDS)) != hipSuccess)              \
                return DDPM_ERR_LAUNCH;                                                                                  \
            attr_set = true;                                                                                             \
        }                                                                                                                \
        hipLaunchKernelGGL((gemm_kernel<T, TA, TB, NB, NWV>), grid, dim3(NWV * 64), (LDS), st, g.A, g.B, g.ep, g.M, g.N, g.K, kps, tiles_n, g_xcd_swizzle, make_fastdiv((unsigned)tiles_n)); \
    } while (0)
    // 8-wave blocks whenever both operands take the DMA path (all bf16 products, fp32 with k-contiguous operands)
    constexpr bool BF = sizeof(T) == 2;
    constexpr int NWT = BF ? 8 : 4;                           // wave count with a k-slow (transposed) operand
    if (!g.A.trans && !g.B.trans) {
        if (deep) LAUNCH(false, false, 5, 8, lds3);
        else LAUNCH(false, false, 2, 8, lds2);
    } else if (!g.A.trans && g.B.trans) {
        LAUNCH(false, true, 2, NWT, lds2);
    } else if (g.A.trans && !g.B.trans) {
        LAUNCH(true, false, 2, NWT, lds2);
    } else {
        if constexpr (BF) {
            if (g.ep.mode >= 2) {          // weight gradients: the scatter-only instantiation
                g.variant = 2;
                if (g.dry) return DDPM_OK;
                static DevOnce attr_set;
                if (!attr_set) {
                    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gemm_kernel<T, true, true, 2, 8, true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds2) != hipSuccess)
                        return DDPM_ERR_LAUNCH;
                    attr_set = true;
                }
                hipLaunchKernelGGL((gemm_kernel<T, true, true, 2, 8, true>), grid, dim3(512), lds2, st, g.A, g.B, g.ep, g.M, g.N, g.K, kps, tiles_n, g_xcd_swizzle, make_fastdiv((unsigned)tiles_n));
            } else LAUNCH(true, true, 2, 8, lds2);
        } else LAUNCH(true, true, 2, 4, lds2);
    }
#undef LAUNCH
    return g.dry ? DDPM_OK : check_launch();
}

static int validate(const MatDesc& d, int esize) {
    if (!d.p) return DDPM_ERR_NULL;
    const int vec = 16 / esize;
    if (!aligned16(d.p)) return DDPM_ERR_ALIGN;
    if (d.ld % vec || d.batch_stride % vec) return DDPM_ERR_ALIGN;
    if (d.conv) { if (d.C % vec) return DDPM_ERR_SHAPE; }
    else if (d.n_fast % vec) return DDPM_ERR_SHAPE;
    return DDPM_OK;
}

static void set_vec_ok(GemmArgs& g, int es) {
    const int vo = g.ep.mode == 0 ? 16 / es : 4;        // elements per 16-byte output vector
    bool ok = aligned16(g.ep.out) && g.ep.ldc % vo == 0 && g.ep.out_batch_stride % vo == 0;
    if (g.ep.residual) ok = ok && aligned16(g.ep.residual) && g.ep.res_ld % (16 / es) == 0 && g.ep.res_batch_stride % (16 / es) == 0;
    g.ep.vec_ok = ok ? 1 : 0;
}

int ddpm_gemm_launch(GemmArgs& g, hipStream_t st) {
    if (g.M <= 0 || g.N <= 0 || g.K <= 0 || g.batch <= 0) return DDPM_ERR_SHAPE;
    if (g.dtype != DDPM_F32 && g.dtype != DDPM_BF16) return DDPM_ERR_DTYPE;
    const int es = g.dtype == DDPM_BF16 ? 2 : 4;
    int rc;
    if ((rc = validate(g.A, es)) != DDPM_OK) return rc;
    if ((rc = validate(g.B, es)) != DDPM_OK) return rc;
    if (!g.ep.out) return DDPM_ERR_NULL;
    if ((rc = finish_desc(g.A, es)) != DDPM_OK) return rc;
    if ((rc = finish_desc(g.B, es)) != DDPM_OK) return rc;
    set_vec_ok(g, es);
    rc = g.dtype == DDPM_BF16 ? launch_t<bf16_t>(g, st) : launch_t<float>(g, st);
    if (g.dry) g_variant_result = g.variant;
    return rc;
}

// ---------------------------------------------------------------------------------------------- C ABI
static void zero_args(GemmArgs& g) { memset(&g, 0, sizeof(g)); g.batch = 1; g.splits = 1; g.ep.alpha = 1.f; g.dry = g_variant_query; }

static void conv_desc(MatDesc& d, const void* x, long long x_ld, int npix_out, int H, int W, int C, int Ho, int Wo, int R, int S,
                      int stride, int pad_t, int pad_l, int upsample, int dilate) {
    d.p = x; d.ld = x_ld; d.batch_stride = 0; d.conv = 1;
    d.n_slow = npix_out; d.n_fast = R * S * C;
    d.conv_batches = npix_out / (Ho * Wo);
    d.H = H; d.W = W; d.C = C; d.Ho = Ho; d.Wo = Wo; d.R = R; d.S = S; d.stride = stride; d.pad_t = pad_t; d.pad_l = pad_l;
    d.sh = (upsample || dilate) ? 1 : 0; d.dmask = dilate ? 1 : 0;
}

// Convolution over NHWC activations as implicit GEMM (forward and, with flipped weights, dgrad).
//   y[b,oy,ox,n] = sum_{r,s,c} x[b, f(oy*stride + r - pad_t), f(ox*stride + s - pad_l), c] * w[n][r][s][c]  (+ epilogue)
// f = identity, >>1 (nearest-2x upsample fused: upsample=1) or /2-if-even (transposed conv: dilate=1).
// splits > 1 (small-M layers): the K range is split over gridDim.y and reduced inside the launch through
// splitk_ws (>= tiles*splits*16384 floats) and splitk_cnt (>= tiles counters, zero on entry and on exit).
extern "C" int ddpm_conv2d_nhwc(const void* x, long long x_ld, const void* w, void* y, long long y_ld,
                                const float* bias, const float* rowbias, long long rowbias_ld,
                                const void* residual, long long res_ld,
                                int B, int H, int W, int C, int Ho, int Wo, int N, int R, int S,
                                int stride, int pad_t, int pad_l, int upsample, int dilate,
                                int accumulate, int out_mode, int splits, float* splitk_ws, unsigned* splitk_cnt,
                                int dtype, void* stream) {
    if (!x || !w || !y) return DDPM_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || Ho <= 0 || Wo <= 0 || N <= 0 || R <= 0 || S <= 0 || stride <= 0) return DDPM_ERR_SHAPE;
    if (upsample && dilate) return DDPM_ERR_SHAPE;
    if (out_mode != 0 && out_mode != 1 && out_mode != 3) return DDPM_ERR_SHAPE;
    GemmArgs g; zero_args(g);
    g.dtype = dtype;
    g.M = B * Ho * Wo; g.N = N; g.K = R * S * C;
    conv_desc(g.A, x, x_ld, g.M, H, W, C, Ho, Wo, R, S, stride, pad_t, pad_l, upsample, dilate);
    g.A.trans = 0;
    g.B.p = w; g.B.ld = g.K; g.B.trans = 0; g.B.n_slow = N; g.B.n_fast = g.K;
    g.ep.out = y; g.ep.ldc = y_ld; g.ep.mode = out_mode; g.ep.bias = bias;
    g.ep.rowbias = rowbias; g.ep.rowbias_ld = rowbias_ld; g.ep.dgroup = make_fastdiv((unsigned)(Ho * Wo));
    g.ep.residual = residual; g.ep.res_ld = res_ld; g.ep.accumulate = accumulate;
    g.ep.HW = Ho * Wo; g.ep.dHW = make_fastdiv((unsigned)(Ho * Wo));
    g.splits = splits; g.ep.splitk_ws = splitk_ws; g.ep.splitk_cnt = splitk_cnt;
    // data gradient of a stride-2 conv (dilate): parity-phase form when every 128-row tile can stay inside one phase — 9/4 taps per output
    // pixel on average instead of 9 over a three-quarters-zero operand.  One K run (the reduction is short), the caller's split offer unused.
    const int bk = dtype == DDPM_BF16 ? 64 : 32;
    if (dilate && R == 3 && S == 3 && stride == 1 && !(Ho & 1) && !(Wo & 1) && C % bk == 0 && (out_mode == 0 || out_mode == 1) &&
        ((long long)B * (Ho / 2) * (Wo / 2)) % TILE == 0) {
        MatDesc& d = g.A;
        d.phase = 1; d.Hh = Ho / 2; d.Wh = Wo / 2; d.Mp = B * d.Hh * d.Wh; d.spt = C / bk;
        d.dMp = make_fastdiv((unsigned)d.Mp); d.dHhWh = make_fastdiv((unsigned)(d.Hh * d.Wh)); d.dWh = make_fastdiv((unsigned)d.Wh);
        d.dSpt = make_fastdiv((unsigned)d.spt);
        g.splits = 1; g.ep.splitk_ws = nullptr; g.ep.splitk_cnt = nullptr;
    }
    // the UNet's edge convs (3 -> hid, hid -> 3) on full-size images: their own kernels (edgeconv.hip)
    if (dtype == DDPM_BF16 && R == 3 && S == 3 && stride == 1 && pad_t == 1 && pad_l == 1 && !upsample && !dilate && Ho == H && Wo == W &&
        !rowbias && !residual && !accumulate && g.M >= 16384) {
        int rc = -1, id = 0;
        if (out_mode == 3 && N <= 16) { rc = ddpm_edgeconv_few_out_launch(x, x_ld, w, y, bias, B, H, W, C, N, g.dry, stream); id = 11; }
        else if (out_mode == 0 && C == 8) { rc = ddpm_edgeconv_few_in_launch(x, x_ld, w, y, y_ld, bias, B, H, W, C, N, g.dry, stream); id = 12; }
        if (rc >= 0) { if (g.dry) { g_variant_result = id; return DDPM_OK; } return rc; }
    }
    // hot case: 3x3 / stride 1 / pad 1 on bf16 -> persistent stationary-halo kernel (conv3x3.hip: 16 x 16 patches, or 8 x 8 for the 8 x 8 level)
    // (`splits` is an offer, not a demand: this kernel needs no split; the nearest-2x up-sampled input of the Upsample blocks is gathered in place)
    if (dtype == DDPM_BF16 && R == 3 && S == 3 && stride == 1 && pad_t == 1 && pad_l == 1 && !dilate && out_mode == 0 &&
        Ho == (H << (upsample ? 1 : 0)) && Wo == (W << (upsample ? 1 : 0))) {
        const int rc = ddpm_conv3x3_stream_launch(x, x_ld, w, y, y_ld, bias, rowbias, rowbias_ld, residual, res_ld, accumulate, B, Ho, Wo, C, N,
                                                  upsample ? 1 : 0, g_xcd_swizzle, g.dry, stream);
        if (rc >= 0) { if (g.dry) { g_variant_result = rc == 8 ? 10 : (rc == 17 ? 13 : 8); return DDPM_OK; } return rc; }
    }
    // ... or the one-tile-per-block form (what conv3x3.hip does not cover)
    constexpr int halo_min_c = 64;
    if (C >= halo_min_c && dtype == DDPM_BF16 && R == 3 && S == 3 && stride == 1 && pad_t == 1 && pad_l == 1 && !upsample && !dilate &&
        out_mode == 0 && splits <= 1 && C % 64 == 0 && Ho == H && Wo == W && g.M >= 16384 && aligned16(x) && aligned16(w) && x_ld % 8 == 0) {
        set_vec_ok(g, 2);
        const int rc = conv3x3_halo_launch(g, x, x_ld, w, B, H, W, C, N, (hipStream_t)stream);
        if (rc >= 0) { if (g.dry) g_variant_result = g.variant; return rc; }     // -1: geometry not covered, fall through to the generic kernel
    }
    // 1x1 / stride 1 on bf16 with a row epilogue the accumulator lanes can do themselves -> persistent streaming kernel (pointwise.hip)
    if (dtype == DDPM_BF16 && R == 1 && S == 1 && stride == 1 && pad_t == 0 && pad_l == 0 && !upsample && !dilate && out_mode == 0 && splits <= 1 &&
        !rowbias && Ho == H && Wo == W) {
        const int rc = ddpm_pointwise_launch(x, x_ld, w, y, y_ld, bias, residual, res_ld, accumulate, g.M, N, C, g.dry, stream);
        if (rc >= 0) { if (g.dry) g_variant_result = 7; return rc; }
    }
    return ddpm_gemm_launch(g, (hipStream_t)stream);
}

// Weight gradient in PACKED layout: dw[n][r][s][c] += sum_{b,oy,ox} dy[b,oy,ox,n] * x[b, f(..), f(..), c]
// (fp32 atomics, n < Nreal, c < Creal; rows of Creal contiguous floats -> coalesced).  ddpm_wgrad_unpack converts
// every layer's packed gradient to the parameter layout [n][c][r][s] in one launch.
// number of split-K slices the kernels really use for a reduction of K with `splits` requested (whole K-steps per slice)
extern "C" int ddpm_wgrad_effective_splits(int K, int splits, int dtype) {
    const int BK = dtype == DDPM_BF16 ? 64 : 32;
    if (K <= 0 || splits < 1) return 1;
    const int ksteps = (K + BK - 1) / BK, steps_per = (ksteps + splits - 1) / splits;
    return (ksteps + steps_per - 1) / steps_per;
}

extern "C" int ddpm_conv2d_wgrad_nhwc(const void* dy, long long dy_ld, const void* x, long long x_ld, float* dw, long long slab_stride,
                                      int B, int H, int W, int C, int Creal, int Ho, int Wo, int N, int Nreal, int R, int S,
                                      int stride, int pad_t, int pad_l, int upsample, int splits, int dtype, void* stream) {
    if (!dy || !x || !dw) return DDPM_ERR_NULL;
    if (B <= 0 || H <= 0 || W <= 0 || C <= 0 || Creal <= 0 || Creal > C || Ho <= 0 || Wo <= 0 || N <= 0 || Nreal <= 0 || Nreal > N) return DDPM_ERR_SHAPE;
    const int vec = dtype == DDPM_BF16 ? 8 : 4;
    if (N % vec) return DDPM_ERR_SHAPE;      // dy is read as 16-byte vectors along n
    GemmArgs g; zero_args(g);
    g.dtype = dtype; g.splits = splits;
    g.M = Nreal; g.N = R * S * C; g.K = B * Ho * Wo;    // dy may carry zero-padded channels beyond Nreal (<= N)
    g.A.p = dy; g.A.ld = dy_ld; g.A.trans = 1; g.A.n_slow = g.K; g.A.n_fast = N;
    conv_desc(g.B, x, x_ld, g.K, H, W, C, Ho, Wo, R, S, stride, pad_t, pad_l, upsample, 0);
    g.B.trans = 1;
    g.ep.out = dw; g.ep.mode = 4; g.ep.Cpad = C; g.ep.Creal = Creal; g.ep.RS = R * S; g.ep.dCpad = make_fastdiv((unsigned)C);
    g.ep.accumulate = 1;      // slab_stride == 0: "+=" with atomics — the caller zero-fills once and may add several contributions
    if (slab_stride > 0) {    // slab mode: split s stores its partial at dw + s*slab_stride; ddpm_wgrad_reduce sums the copies
        if (slab_stride < (long long)Nreal * R * S * Creal || splits != ddpm_wgrad_effective_splits(g.K, splits, dtype)) return DDPM_ERR_SHAPE;
        g.ep.mode = 5; g.ep.slab_stride = slab_stride;
    } else if (slab_stride < 0) return DDPM_ERR_SHAPE;
    return ddpm_gemm_launch(g, (hipStream_t)stream);
}

// Batched GEMM  C[b][m][n] = alpha * sum_k A[b][m][k] * B[b][n][k]  (+bias[n]) (+residual) (+= when accumulate).
// a_trans / b_trans = 1 when the operand is stored with k as the slow index ([k][m] / [k][n]).
// out_mode: 0 store dtype | 1 store fp32 | 2 atomic-add fp32 (required when splits > 1).
extern "C" int ddpm_gemm(const void* a, long long a_ld, long long a_bs, int a_trans,
                         const void* b, long long b_ld, long long b_bs, int b_trans,
                         void* c, long long c_ld, long long c_bs,
                         const float* bias, const void* residual, long long res_ld, long long res_bs,
                         int M, int N, int K, int batch, float alpha, int accumulate, int out_mode, int splits,
                         int dtype, void* stream) {
    if (!a || !b || !c) return DDPM_ERR_NULL;
    if (out_mode < 0 || out_mode > 2) return DDPM_ERR_SHAPE;
    GemmArgs g; zero_args(g);
    g.dtype = dtype; g.M = M; g.N = N; g.K = K; g.batch = batch; g.splits = splits;
    g.A.p = a; g.A.ld = a_ld; g.A.batch_stride = a_bs; g.A.trans = a_trans;
    g.A.n_slow = a_trans ? K : M; g.A.n_fast = a_trans ? M : K;
    g.B.p = b; g.B.ld = b_ld; g.B.batch_stride = b_bs; g.B.trans = b_trans;
    g.B.n_slow = b_trans ? K : N; g.B.n_fast = b_trans ? N : K;
    g.ep.out = c; g.ep.ldc = c_ld; g.ep.out_batch_stride = c_bs; g.ep.mode = out_mode; g.ep.alpha = alpha;
    g.ep.bias = bias; g.ep.residual = residual; g.ep.res_ld = res_ld; g.ep.res_batch_stride = res_bs;
    g.ep.accumulate = accumulate;
    return ddpm_gemm_launch(g, (hipStream_t)stream);
}

// Fused attention forward over a packed qkv buffer [B][L][ld] (q at channel 0, k at C, v at 2C): out[B][L][out_ld] =
// softmax(q k^T * scale) v.  bf16 only; C in {128, 256}; L a multiple of 128.  Other geometries: DDPM_ERR_SHAPE (the
// caller keeps the three-launch path for them).
extern "C" int ddpm_attention_fwd(const void* qkv, long long ld, void* out, long long out_ld, int B, int L, int C, float scale,
                                  int dtype, void* stream) {
    if (!qkv || !out) return DDPM_ERR_NULL;
    if (dtype != DDPM_BF16) return DDPM_ERR_DTYPE;
    if (B <= 0 || L <= 0 || L % 128 || (C != 128 && C != 256) || ld < 3 * C) return DDPM_ERR_SHAPE;
    if (!aligned16(qkv) || !aligned16(out) || ld % 8 || out_ld % 8) return DDPM_ERR_ALIGN;
    MatDesc q, k, v;
    memset(&q, 0, sizeof(q));
    q.p = qkv; q.ld = ld; q.batch_stride = (long long)L * ld; q.trans = 0; q.n_slow = L; q.n_fast = C;
    k = q; k.p = (const bf16_t*)qkv + C;
    v = q; v.p = (const bf16_t*)qkv + 2 * C; v.trans = 1; v.n_slow = L; v.n_fast = C;
    if (finish_desc(q, 2) || finish_desc(k, 2) || finish_desc(v, 2)) return DDPM_ERR_SHAPE;
    const int DC = C / 64, VT = C / 128;
    const int lds = DC * TILE * ROW_BYTES + DC * 64 * ROW_BYTES + VT * 64 * 256;
    const dim3 grid(L / 128, B);
    hipStream_t st = (hipStream_t)stream;
    if (C == 256) {
        static DevOnce attr;
        if (!attr) { if (hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_kernel<8>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return DDPM_ERR_LAUNCH; attr = true; }
        hipLaunchKernelGGL(attn_fwd_kernel<8>, grid, dim3(256), lds, st, q, k, v, (bf16_t*)out, out_ld, L, scale);
    } else {
        static DevOnce attr;
        if (!attr) { if (hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_fwd_kernel<4>), hipFuncAttributeMaxDynamicSharedMemorySize, lds) != hipSuccess) return DDPM_ERR_LAUNCH; attr = true; }
        hipLaunchKernelGGL(attn_fwd_kernel<4>, grid, dim3(256), lds, st, q, k, v, (bf16_t*)out, out_ld, L, scale);
    }
    return check_launch();
}

// ---- which kernel would serve this call?  Same argument meaning as the launching entry points, no pointers, nothing launched,
// no state: returns the kernel id (see the top of the host section) or -(error code).
static const void* const FAKE = reinterpret_cast<const void*>(0x1000);

extern "C" int ddpm_conv2d_variant(long long x_ld, long long y_ld, int B, int H, int W, int C, int Ho, int Wo, int N, int R, int S,
                                   int stride, int pad_t, int pad_l, int upsample, int dilate, int out_mode, int splits, int dtype, int epilogue) {
    // epilogue: bit 0 = the call has a residual operand, bit 1 = it accumulates into y (the 3x3 dispatch depends on them)
    g_variant_query = 1;
    const int rc = ddpm_conv2d_nhwc(FAKE, x_ld, FAKE, const_cast<void*>(FAKE), y_ld, nullptr, nullptr, 0, (epilogue & 1) ? FAKE : nullptr, (epilogue & 1) ? y_ld : 0, B, H, W, C, Ho, Wo, N, R, S, stride, pad_t, pad_l,
                                    upsample, dilate, (epilogue >> 1) & 1, out_mode, splits, splits > 1 ? reinterpret_cast<float*>(0x1000) : nullptr,
                                    splits > 1 ? reinterpret_cast<unsigned*>(0x1000) : nullptr, dtype, nullptr);
    const int v = g_variant_result;
    g_variant_query = 0;
    return rc ? -rc : v;
}
extern "C" int ddpm_conv2d_wgrad_variant(long long dy_ld, long long x_ld, int B, int H, int W, int C, int Creal, int Ho, int Wo, int N, int Nreal,
                                         int R, int S, int stride, int pad_t, int pad_l, int upsample, int splits, int dtype) {
    g_variant_query = 1;
    const int rc = ddpm_conv2d_wgrad_nhwc(FAKE, dy_ld, FAKE, x_ld, reinterpret_cast<float*>(0x1000), 0, B, H, W, C, Creal, Ho, Wo, N, Nreal, R, S, stride, pad_t, pad_l,
                                          upsample, splits, dtype, nullptr);
    const int v = g_variant_result;
    g_variant_query = 0;
    return rc ? -rc : v;
}
extern "C" int ddpm_gemm_variant(long long a_ld, int a_trans, long long b_ld, int b_trans, long long c_ld, int M, int N, int K, int batch,
                                 int out_mode, int splits, int dtype) {
    g_variant_query = 1;
    const int rc = ddpm_gemm(FAKE, a_ld, 0, a_trans, FAKE, b_ld, 0, b_trans, const_cast<void*>(FAKE), c_ld, 0, nullptr, nullptr, 0, 0, M, N, K, batch, 1.f, 0, out_mode,
                             splits, dtype, nullptr);
    const int v = g_variant_result;
    g_variant_query = 0;
    return rc ? -rc : v;
}
