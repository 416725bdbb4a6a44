// The bf16 operand view shared by the attention kernel files (attention.hip, attention_stream.hip): one image's rows behind a raw
// buffer descriptor, its 16-byte load and the MFMA fragment cast.  Included after common.h.
#pragma once

struct Opnd {                                   // [L rows][C] bf16, row pitch ld (elements); rsrc spans one image
    __amdgpu_buffer_rsrc_t rsrc;
    long long ld;
};
__device__ __forceinline__ Opnd make_opnd(const bf16_t* base, long long ld, int L, int C) {
    Opnd o;
    const UniformAddr u = uniform_addr(base);
    o.rsrc = buffer_rsrc_at(u, (unsigned)(((long long)(L - 1) * ld + C) * 2));
    o.ld = ld;
    return o;
}
__device__ __forceinline__ u32x4 ldv(const Opnd& o, unsigned off) {
    return __builtin_bit_cast(u32x4, __builtin_amdgcn_raw_buffer_load_b128(o.rsrc, off, 0, 0));
}
__device__ __forceinline__ bf16x8 as_frag(const u32x4& v) { return __builtin_bit_cast(bf16x8, v); }
