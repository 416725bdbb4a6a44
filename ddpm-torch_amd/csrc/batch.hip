// Batch assembly for a data set that lives on the device (ddpm_torch/datasets.py DeviceLoader): out[b] = transform(data[index[b]]),
// one launch per batch — gather by index, uint8 -> float through a 256-entry table, random horizontal flip.
//
// The data set can be larger than 4 GiB (CelebA-HQ as uint8 is 5.9 GB), so nothing here goes through a buffer descriptor: an image's
// base is 64-bit arithmetic on the plain global pointer, and only the offset INSIDE one image (C*H*W < 2^31, checked on the host)
// is 32-bit.  The work is a few MB per batch; there is one kernel in two forms and no tuning in it.
#include "common.h"
#include "../../include/ddpm_hip.h"

// One work item = one 16-byte group of a source row (WIDE: 16 bytes or 4 floats, rows are whole groups and every base is 16-byte
// aligned) or one element (any other geometry).  A mirrored row reads the mirrored item and, WIDE, reverses it in registers, so loads
// and stores keep their width either way.  blockIdx.x walks the items of one image, blockIdx.y the samples.
template <typename T, bool WIDE>
__global__ __launch_bounds__(256) void batch_gather_kernel(const T* __restrict__ data, const long long* __restrict__ index,
                                                           const float* __restrict__ lut, float* __restrict__ out, int B, long long n_images,
                                                           int chw, int W, int flip, unsigned long long seed) {
    constexpr bool BYTES = sizeof(T) == 1;
    constexpr int VEC = WIDE ? 16 / (int)sizeof(T) : 1;
    __shared__ float s_lut[256];
    if constexpr (BYTES) {
        s_lut[threadIdx.x] = lut[threadIdx.x];
        __syncthreads();
    }
    // unsigned: items can be up to 2^31 - 1, and the last block's item numbers run up to 255 past it
    const unsigned items = (unsigned)chw / VEC, row_items = (unsigned)W / VEC;
    const unsigned u = blockIdx.x * 256u + threadIdx.x;
    if (u >= items) return;
    const unsigned k = u % row_items;
    const unsigned u_mirror = u - k + (row_items - 1 - k);
    const float nan = __builtin_nanf("");
    for (int b = blockIdx.y; b < B; b += gridDim.y) {
        const long long idx = index[b];
        float* dst = out + (long long)b * chw + (long long)u * VEC;
        if (idx < 0 || idx >= n_images) {                                       // as ddpm_q_sample does for a t outside its tables
            if constexpr (WIDE) {
                for (int j = 0; j < VEC; j += 4) *reinterpret_cast<f32x4*>(dst + j) = (f32x4)(nan);
            } else {
                *dst = nan;
            }
            continue;
        }
        const bool mirror = flip && (dropout_word(seed, (unsigned long long)idx) >> 31);
        const T* src = data + idx * chw + (long long)(mirror ? u_mirror : u) * VEC;
        if constexpr (!WIDE) {
            if constexpr (BYTES) *dst = s_lut[*src]; else *dst = *src;
        } else {
            u32x4 v = ldg16(src);
            if constexpr (BYTES) {
                if (mirror) {
                    const u32x4 r = v;
                    v.x = __builtin_bswap32(r.w); v.y = __builtin_bswap32(r.z); v.z = __builtin_bswap32(r.y); v.w = __builtin_bswap32(r.x);
                }
                const unsigned words[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    f32x4 o;
                    o.x = s_lut[words[j] & 255u]; o.y = s_lut[(words[j] >> 8) & 255u]; o.z = s_lut[(words[j] >> 16) & 255u]; o.w = s_lut[words[j] >> 24];
                    *reinterpret_cast<f32x4*>(dst + 4 * j) = o;
                }
            } else {
                if (mirror) {
                    const u32x4 r = v;
                    v.x = r.w; v.y = r.z; v.z = r.y; v.w = r.x;
                }
                stg16(dst, v);
            }
        }
    }
}

template <typename T>
static void batch_gather_launch(const void* data, const long long* index, const float* lut, float* out, int B, long long n_images, int chw, int W,
                                int flip, unsigned long long seed, hipStream_t st) {
    constexpr int VEC = 16 / (int)sizeof(T);
    // chw is a multiple of VEC whenever W is, so with aligned bases every image and every output sample starts on a 16-byte boundary
    const bool wide = W % VEC == 0 && aligned16(data) && aligned16(out);
    const unsigned items = wide ? (unsigned)chw / VEC : (unsigned)chw;
    const dim3 grid((items + 255u) / 256u, B < 65535 ? B : 65535);
    if (wide) hipLaunchKernelGGL((batch_gather_kernel<T, true>), grid, dim3(256), 0, st, (const T*)data, index, lut, out, B, n_images, chw, W, flip, seed);
    else hipLaunchKernelGGL((batch_gather_kernel<T, false>), grid, dim3(256), 0, st, (const T*)data, index, lut, out, B, n_images, chw, W, flip, seed);
}

extern "C" int ddpm_batch_gather(const void* data, int src_dtype, const long long* index, const float* lut, float* out,
                                 int B, long long n_images, int C, int H, int W, int flip, unsigned long long seed, void* stream) {
    if (src_dtype != 0 && src_dtype != 1) return DDPM_ERR_DTYPE;
    if (!data || !index || !out || (src_dtype == 0 && !lut)) return DDPM_ERR_NULL;
    if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || n_images <= 0) return DDPM_ERR_SHAPE;
    const long long ch = (long long)C * H, chw = ch * W;                       // ch < 2^62; checked before chw can overflow
    if (ch >= (1ll << 31) || chw >= (1ll << 31)) return DDPM_ERR_SHAPE;
    if (src_dtype == 0) batch_gather_launch<unsigned char>(data, index, lut, out, B, n_images, (int)chw, W, flip, seed, (hipStream_t)stream);
    else batch_gather_launch<float>(data, index, lut, out, B, n_images, (int)chw, W, flip, seed, (hipStream_t)stream);
    return check_launch();
}
