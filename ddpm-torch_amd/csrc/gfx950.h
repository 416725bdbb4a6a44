// gfx950 device primitives shared by the kernel files: buffer descriptors, LDS-DMA, counted waits, asm LDS reads, the XCD block order
// and the LDS counter semaphores of the wave-specialised kernels.  Included by common.h; every caveat is written here once.
#pragma once

template <int I> struct IC { static constexpr int v = I; };
// f(IC<0>{}), ..., f(IC<N - 1>{}): a loop whose index is a compile-time constant inside the body (asm immediates, template arguments)
template <int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (N > 0) { static_for<N - 1>(f); f(IC<N - 1>{}); }
}

// XCD-aware block order.  Workgroups are handed to the 8 XCDs round-robin by linear id, and each XCD has its own L2: with the
// natural order the blocks that share operand data (the N-tiles of one pixel tile, the output tiles of one split-K slice) sit
// on 8 different XCDs and every L2 fetches the same lines again (measured on wgrad: the LDS-DMA stream alone took as long
// as the whole kernel).  Logical id = (id % 8) * (total / 8) + id / 8 gives each XCD a CONTIGUOUS range of logical ids, so
// neighbours in the logical order — which share data — run on the same XCD at about the same time.  The (< 8) ids past
// the last multiple of 8 keep their own id.  xcd = 0 is the natural order; the kernels without the argument pass 1.
__device__ __forceinline__ int xcd_logical_id(int id, int total, int xcd) {
    if (!xcd) return id;
    const int per = total >> 3;
    return id < (per << 3) ? (id & 7) * per + (id >> 3) : id;
}

// ---- buffer descriptors.  All streamed global reads go through a raw buffer descriptor (base, num_records = extent in bytes): addressing
// is one 32-bit byte offset per lane and the hardware range check returns ZEROS (drops the write) for any offset >= num_records —
// also for the direct-to-LDS form (scripts/probes/buffer_lds_oob.hip).  BUF_OOB is the offset a lane without data uses; BUF_OOB plus a
// small in-tile offset stays out of range, and it is the launchers' limit for an operand's extent.
constexpr unsigned BUF_OOB = 0x7ffffff0u;
// The descriptor must be PROVABLY wave-uniform or hipcc wraps every buffer op in a waterfall loop (v_readfirstlane x4 +
// s_and_saveexec per load): readfirstlane its inputs once.  readfirstlane returns INT: each half of the address is assigned to an
// `unsigned` before the two are joined — OR-ed into the 64-bit base as it comes, the low half sign-extends and the descriptor points at
// 0xffff.... whenever bit 31 of the address is set (every load then returns the range check's zeros; DESIGN.md section 4, "1x1").
struct UniformAddr { unsigned lo, hi; };
__device__ __forceinline__ UniformAddr uniform_addr(const void* p) {
    const unsigned long long ad = (unsigned long long)p;
    const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)ad), hi = __builtin_amdgcn_readfirstlane((unsigned)(ad >> 32));
    return UniformAddr{lo, hi};
}
// (the two steps are separate for attention_common.h's make_opnd, which works out the extent between them; everyone else calls buffer_rsrc)
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc_at(UniformAddr base, unsigned extent) {
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((unsigned long long)base.hi << 32) | base.lo), 0,
                                             __builtin_amdgcn_readfirstlane((int)extent), 0x00020000);
}
__device__ __forceinline__ __amdgpu_buffer_rsrc_t buffer_rsrc(const void* p, unsigned extent) { return buffer_rsrc_at(uniform_addr(p), extent); }

// byte address inside the workgroup's LDS of a pointer into `extern __shared__`: what the asm reads and the semaphores below take
__device__ __forceinline__ unsigned lds_addr(const void* smem) {
    return (unsigned)(size_t)smem;
}
// LDS-DMA (`buffer_load_dwordx4 ... lds`): 16 bytes per lane from rsrc[voffset + soffset] to lds_dst + 16 * lane, without touching VGPRs.
// lds_dst (a pointer into `extern __shared__`) and soffset are wave-uniform; counted by vmcnt like any load (loads retire in order).
// A macro, not a function: the passes that run before the inliner would see an opaque call in place of an intrinsic whose memory
// effects they know, and what they leave behind differs (as a function it changed the code of gn_lds_bwd8_kernel<float, 8>).
#define LDS_DMA16(rsrc, lds_dst, voffset, soffset) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (__attribute__((address_space(3))) void*)(lds_dst), 16, voffset, soffset, 0, 0)
template <int N> __device__ __forceinline__ void wait_vm() {
    static_assert(N >= 0 && N < 64, "vmcnt immediate");
    asm volatile("s_waitcnt vmcnt(%0)" :: "n"(N) : "memory");
}

// ---- LDS reads next to an LDS-DMA in flight are inline asm: hipcc puts `s_waitcnt vmcnt(0)` in front of any ds_read it generates while
// a DMA may be outstanding (it cannot tell which bytes the DMA writes), which would drain the ring at every step.  These return before
// the data has: the caller waits (lds_wait / lds_wait_n) before the first use.
__device__ __forceinline__ u32x4 lds_rd16(unsigned addr) {
    u32x4 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
// hardware transpose read (ds_read_b64_tr_b16): the 16-lane group's lanes 4r..4r+3 address 4 k-rows x (4 x 8 bytes); lane c receives,
// for its column c of the 16 columns, the 4 k values (see read_frag<T, true> in gemm.hip)
__device__ __forceinline__ uint2 lds_rd_tr(unsigned addr) {
    uint2 v;
    asm volatile("ds_read_b64_tr_b16 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
// the same read as a builtin, for kernels whose LDS reads the compiler may track (it then places the waits itself)
__device__ __forceinline__ uint2 tr_read(const char* p) {
    const s16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(p));
    return __builtin_bit_cast(uint2, v);
}
// (the fence keeps hipcc from moving an MFMA, which depends on the reads' registers but not on the wait, ahead of it)
__device__ __forceinline__ void lds_wait() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0); }
template <int N> __device__ __forceinline__ void lds_wait_n() { asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(N) : "memory"); __builtin_amdgcn_sched_barrier(0); }

// ---- counter semaphores in LDS: how the loader and consumer waves of a wave-specialised kernel (conv3x3_pc_kernel, wgrad3x3_ws_kernel)
// meet without s_barrier.  (wgrad.hip still spells lds_wait_all_ge's loop itself, as ws_wait_all_ge: this spelling moves the registers
// around its wait loops, its spelling those of conv3x3_pc_kernel, and a kernel that changes has to be timed on the GPU first.)
//   * Every counter has a SINGLE WRITER (one wave) and only grows; a waiter compares by wrap-safe signed distance.
//   * ONE COUNTER PER SIGNALLING WAVE, never a sum over waves: a wave that runs a step ahead of its siblings would otherwise make up for
//     a sibling's missing signal (`ready >= 4 (s + 1)` held with one loader's quarter of the tile still in flight: a rare wrong tile when
//     the block's waves progress unevenly, e.g. next to another kernel).  The four counters of a group are 16 contiguous bytes: one
//     ds_read_b128 returns all four, the poller takes the minimum (lds_wait_all_ge).  A summed counter is only sound where the waiters
//     need ALL signallers of one round and nobody can run a round ahead (lds_wait_ge: the consumers' rendezvous).
//   * A wave signals with one unmasked LDS write: lane 0 on the counter, every other lane on its own word of a junk area
//     (no exec masking, no bank conflict); `lane_addr` is built once per wave.
//   * The waits are bounded: a protocol error must end the launch with an error the host sees (trap), never hang the GPU.  The bound is
//     WALL time (s_memrealtime, 100 MHz): ~5 s, so that a profiler's thread trace or a stalled co-tenant cannot turn a slow wait
//     into a fault; the clock is looked at every 4096 polls only.  Before the trap {block, counter address, target, 1 + kind} is left in
//     `fault` (4 words of device memory owned by the kernel's file; kind 0: lds_wait_all_ge, 1: lds_wait_ge), which a core file names
//     and the file's ddpm_*_last_fault reads where the context survives.
constexpr unsigned long long LDS_WAIT_TICKS = 500000000ull;          // 5 s of the 100 MHz s_memrealtime clock
// the smallest of four counters is >= target (wrap-safe signed distance)
__device__ __forceinline__ int lds_min_dist(const u32x4& v, unsigned target) {
    const int a = (int)(v.x - target), b = (int)(v.y - target), c = (int)(v.z - target), d = (int)(v.w - target);
    const int m = min(min(a, b), min(c, d));
    return __builtin_amdgcn_readfirstlane(m);
}
__device__ __forceinline__ bool lds_wait_expired(unsigned long long& t_first) {
    const unsigned long long now = wall_clock64();
    if (t_first == 0) { t_first = now | 1ull; return false; }
    return now - t_first > LDS_WAIT_TICKS;
}
__device__ __forceinline__ void lds_wait_fault(unsigned* fault, unsigned addr, unsigned target, unsigned kind) {
    if ((threadIdx.x & 63) == 0) {
        fault[0] = blockIdx.x; fault[1] = addr; fault[2] = target; fault[3] = 1u + kind;
        __threadfence_system();
    }
    __builtin_trap();
}
__device__ __forceinline__ void lds_wait_all_ge(unsigned* fault, unsigned addr, unsigned target) {
    unsigned long long t_first = 0;
    for (unsigned spins = 0;; ++spins) {
        u32x4 v;
        asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr) : "memory");
        if (lds_min_dist(v, target) >= 0) break;
        if ((spins & 4095u) == 4095u && lds_wait_expired(t_first)) lds_wait_fault(fault, addr, target, 0u);
        __builtin_amdgcn_s_sleep(1);
    }
}
__device__ __forceinline__ void lds_wait_ge(unsigned* fault, unsigned addr, unsigned target) {
    unsigned long long t_first = 0;
    for (unsigned spins = 0;; ++spins) {
        unsigned v;
        asm volatile("ds_read_b32 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=&v"(v) : "v"(addr) : "memory");
        if ((int)((unsigned)__builtin_amdgcn_readfirstlane((int)v) - target) >= 0) break;
        if ((spins & 4095u) == 4095u && lds_wait_expired(t_first)) lds_wait_fault(fault, addr, target, 1u);
        __builtin_amdgcn_s_sleep(1);
    }
}
// +1 on a counter (ds_add_u32 of the whole wave)
__device__ __forceinline__ void lds_signal(unsigned lane_addr) {
    const unsigned one = 1u;
    asm volatile("ds_add_u32 %0, %1" :: "v"(lane_addr), "v"(one) : "memory");
}
// a wave sets its counter to `value` (ds_write_b32 of the whole wave)
__device__ __forceinline__ void lds_publish(unsigned lane_addr, unsigned value) {
    asm volatile("ds_write_b32 %0, %1" :: "v"(lane_addr), "v"(value) : "memory");
}
