// Launch-plan executor: the training step's ~490 C-ABI calls recorded once, re-issued by ONE call per plan segment.
//
// Why: `Trainer.step` (ddpm_torch/utils/train.py:148-170 upstream) is a fixed, shape-static sequence of launches; issuing it from
// Python costs 6-7 ms of interpreter + ctypes time per ~9.4 ms GPU step, and a replayed hipGraph serialises the two streams the step
// uses (main chain | weight-gradient leaves).  A plan keeps EAGER semantics — every entry is the same `ddpm_*` call with the same
// arguments on the same hipStream_t, the side stream stays concurrent, RCCL calls run between segments — and takes the interpreter out.
//
// An entry = (thunk of an exported `int ddpm_xxx(...)`, its arguments as 64-bit words).  The thunks are generated from the declarations
// in include/ddpm_hip.h by a variadic template, so an entry point whose signature changes cannot be called with a stale layout: the
// argument count is checked when the entry is appended.  Nothing here allocates device memory or synchronises.
#include "common.h"
#include "../../include/ddpm_hip.h"
#include "../../include/ddpm_hip_debug.h"

#include <cstring>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

namespace {

typedef unsigned long long word_t;

template <class T> inline T from_word(word_t w) {
    if constexpr (std::is_pointer<T>::value) {
        return reinterpret_cast<T>(static_cast<uintptr_t>(w));
    } else if constexpr (std::is_same<T, float>::value) {
        const unsigned u = static_cast<unsigned>(w);
        float f;
        std::memcpy(&f, &u, 4);
        return f;
    } else {
        return static_cast<T>(w);            // int (two's complement in the low 32 bits), long long, unsigned long long
    }
}

typedef int (*thunk_t)(const word_t*);

template <class... A, size_t... I> inline int invoke(int (*fn)(A...), const word_t* w, std::index_sequence<I...>) {
    return fn(from_word<A>(w[I])...);
}
template <class R, class... A> constexpr int arity(R (*)(A...)) { return (int)sizeof...(A); }
template <class... A> inline int invoke_all(int (*fn)(A...), const word_t* w) { return invoke(fn, w, std::index_sequence_for<A...>{}); }

// what an entry point puts on its stream (always its LAST argument): kernels through the launch wrapper of common.h, something else
// the wrapper never sees (a memset), or nothing at all (ddpm_stream_order, whose two arguments are both streams).  EP_SIZING: a
// workspace-size query that belongs to a launching entry of this table — listed so that ddpm_plan_entry_arity can tell a recorder the
// argument count it was declared with, never appended to a plan (it enqueues nothing and its value is not a status)
enum EntryKind { EP_KERNELS, EP_ENQUEUES, EP_EDGE, EP_SIZING };

struct EntryPoint {
    const char* name;
    thunk_t thunk;
    int nargs;
    EntryKind kind;
};

#define EP(fn) {#fn, [](const word_t* w) -> int { return invoke_all(&fn, w); }, arity(&fn), EP_KERNELS}
#define EP_AS(fn, kind) {#fn, [](const word_t* w) -> int { return invoke_all(&fn, w); }, arity(&fn), kind}
#define EP_SIZE_OF(fn) {#fn, nullptr, arity(&fn), EP_SIZING}

}  // namespace

extern "C" int ddpm_stream_order(void* waiter, void* signaller);
extern "C" int ddpm_fill_zero(void* p, long long bytes, void* stream);

namespace {

// every launching entry point of include/ddpm_hip.h (the pure queries — *_variant, *_splits, ddpm_gn_workspace_floats — enqueue nothing)
const EntryPoint kEntryPoints[] = {
    EP(ddpm_conv2d_nhwc), EP(ddpm_conv2d_wgrad_nhwc), EP(ddpm_conv3x3_wgrad_nhwc), EP(ddpm_conv3x3_wgrad_up_nhwc), EP(ddpm_conv1x1_wgrad_nhwc),
    EP(ddpm_wgrad_reduce), EP(ddpm_wgrad_unpack), EP(ddpm_wgrad_unpack_sumsq), EP(ddpm_gemm),
    EP(ddpm_attention_fwd), EP(ddpm_attention_fwd_lse), EP(ddpm_attention_bwd), EP(ddpm_attention_stream_fwd), EP(ddpm_attention_stream_bwd),
    EP(ddpm_attention_mh_fwd), EP(ddpm_attention_mh_bwd),
    EP(ddpm_groupnorm_silu_fwd),
    EP(ddpm_groupnorm_silu_bwd), EP(ddpm_timestep_embedding), EP(ddpm_nchw_to_nhwc), EP(ddpm_pack_weight), EP(ddpm_pack_weight_multi),
    EP(ddpm_q_sample), EP(ddpm_mse_fwd), EP(ddpm_mse_bwd), EP(ddpm_weighted_sum_f32), EP(ddpm_atb_f32), EP(ddpm_p_sample_step), EP(ddpm_vlb_terms), EP(ddpm_vlb_terms_bwd), EP(ddpm_gather_i64),
    EP(ddpm_add_i64), EP(ddpm_gather_rows_f32), EP(ddpm_silu_fwd), EP(ddpm_silu_bwd), EP(ddpm_colsum), EP(ddpm_upsample2x_bwd), EP(ddpm_resample2x_nhwc),
    EP(ddpm_add_rows), EP(ddpm_softmax_fwd), EP(ddpm_softmax_bwd), EP(ddpm_sumsq_accumulate), EP(ddpm_adam_ema_step), EP(ddpm_mt_grad_sumsq),
    EP(ddpm_mt_adam_ema), EP(ddpm_mt_gather_f32), EP(ddpm_mfma_probe), EP(ddpm_copy_probe), EP(ddpm_dropout_mask), EP_AS(ddpm_stream_order, EP_EDGE), EP_AS(ddpm_fill_zero, EP_ENQUEUES),
    EP(ddpm_toy_time_table), EP(ddpm_toy_decoder_fwd), EP(ddpm_toy_decoder_bwd), EP(ddpm_toy_time_table_bwd),
    EP(ddpm_manifold_kth_f16), EP(ddpm_manifold_cover_f16), EP(ddpm_bpd_terms), EP(ddpm_bpd_finish), EP(ddpm_batch_gather),
    EP(ddpm_ddim_encode_step), EP(ddpm_slerp), EP_SIZE_OF(ddpm_slerp_workspace_floats),
    EP(ddpm_p_sample_step_lv), EP(ddpm_vlb_terms_lv), EP(ddpm_bpd_terms_lv), EP(ddpm_learned_loss),
    EP(ddpm_class_embed_fwd), EP(ddpm_class_embed_bwd), EP(ddpm_p_sample_step_cfg),
    EP(ddpm_groupnorm_mod_silu_fwd), EP(ddpm_groupnorm_mod_silu_bwd),
    EP(ddpm_p_sample_step_masked), EP(ddpm_q_jump),
};
constexpr int kNumEntryPoints = (int)(sizeof(kEntryPoints) / sizeof(kEntryPoints[0]));

// How the executor issues one entry (resolved per segment, see resolve()):
//   RUN       call the thunk, nothing else
//   PRODUCER  a later edge of the segment waits for this entry's kernels: the thunk runs with a pooled event armed for its stream, and the
//             launch wrapper (common.h) attaches the event to every kernel the entry launches there — the last one is what a wait binds to
//   WAIT      an edge whose producer is entry `producer`: hipStreamWaitEvent on that entry's event only, no marker on the signaller
//   RECORD    an edge with no producing kernel launch in its segment: hipEventRecord + hipStreamWaitEvent, as an eager call does
//   SKIP      an edge that orders nothing: no entry has enqueued on its signaller since the previous edge with the same two streams
enum Mode : unsigned char { RUN, PRODUCER, WAIT, RECORD, SKIP };

struct Entry {
    thunk_t thunk;
    int first_word;       // index into Plan::words
    int ep;               // index into kEntryPoints (for diagnostics)
    Mode mode = RUN;
    int producer = -1;    // WAIT: index of the entry whose event the edge waits for
};

struct Plan {
    std::vector<Entry> entries;
    std::vector<word_t> words;
    std::vector<int> segment_end;     // entries [segment_end[s-1], segment_end[s]) form segment s; the open segment ends at entries.size()
    std::vector<hipEvent_t> bound;    // per entry: the event its kernels carried in the run under way (PRODUCER entries; nullptr = none launched)
    size_t resolved_entries = 0, resolved_cuts = 0;      // what resolve() last saw: appending or cutting re-resolves
    int failed_index = -1;
    int failed_status = 0;
};

// ---- events for ddpm_stream_order: a per-device ring, created on first use, never destroyed (process lifetime).  Re-recording an event
// that an earlier hipStreamWaitEvent still refers to is well defined: a wait binds to the record that precedes it in program order.
constexpr int kRing = 2048;
struct EventRing {
    hipEvent_t ev[kRing];
    std::atomic<unsigned> next{0};
    bool ready = false;
};
EventRing g_rings[64];
std::mutex g_ring_mutex;             // guards the creation of a ring; taking an event from a ready ring needs no lock

// the calling device's ring, its events created on first use (nullptr: the runtime refused)
EventRing* ring_of_device() {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    EventRing& r = g_rings[dev & 63];
    std::lock_guard<std::mutex> lock(g_ring_mutex);
    if (!r.ready) {
        for (int i = 0; i < kRing; ++i)
            if (hipEventCreateWithFlags(&r.ev[i], hipEventDisableTiming) != hipSuccess) return nullptr;
        r.ready = true;
    }
    return &r;
}
inline hipEvent_t next_event(EventRing& r) { return r.ev[r.next.fetch_add(1, std::memory_order_relaxed) % kRing]; }

inline int record_and_wait(EventRing& r, hipStream_t waiter, hipStream_t signaller) {
    const hipEvent_t e = next_event(r);
    if (hipEventRecord(e, signaller) != hipSuccess) return DDPM_ERR_LAUNCH;
    if (hipStreamWaitEvent(waiter, e, 0) != hipSuccess) return DDPM_ERR_LAUNCH;
    return DDPM_OK;
}

// Bind every edge of the plan to the entry that produces what it orders.  Per segment (the host may enqueue anything between two
// segments, so nothing is resolved across a cut): walk back from the edge to the last entry that enqueues on its signaller.
void resolve(Plan* p) {
    const int n = (int)p->entries.size();
    const word_t* words = p->words.data();
    for (Entry& e : p->entries) { e.mode = RUN; e.producer = -1; }
    size_t seg = 0;
    int first = 0;
    for (int i = 0; i < n; ++i) {
        while (seg < p->segment_end.size() && p->segment_end[seg] <= i) first = p->segment_end[seg++];
        Entry& e = p->entries[i];
        if (kEntryPoints[e.ep].kind != EP_EDGE) continue;
        const word_t waiter = words[e.first_word], signaller = words[e.first_word + 1];
        if (waiter == signaller) continue;                       // the call itself is a no-op
        e.mode = RECORD;
        for (int j = i - 1; j >= first; --j) {
            const Entry& q = p->entries[j];
            const EntryPoint& ep = kEntryPoints[q.ep];
            if (ep.kind == EP_EDGE) {
                if (words[q.first_word] == waiter && words[q.first_word + 1] == signaller) { e.mode = SKIP; break; }
                if (words[q.first_word] == signaller && words[q.first_word + 1] != signaller) break;   // the signaller itself waits there: only a record behind that wait carries it along
                continue;
            }
            if (words[q.first_word + ep.nargs - 1] != signaller) continue;
            if (ep.kind == EP_KERNELS) { e.mode = WAIT; e.producer = j; }
            break;
        }
        if (e.mode == WAIT) p->entries[e.producer].mode = PRODUCER;
    }
    p->bound.assign(n, nullptr);
    p->resolved_entries = p->entries.size();
    p->resolved_cuts = p->segment_end.size();
}

}  // namespace

thread_local DdpmLaunchEdge g_ddpm_launch_edge;

extern "C" {

/* `waiter` (a hipStream_t) will not run anything enqueued after this call before everything enqueued on `signaller` so far has finished:
 * hipEventRecord + hipStreamWaitEvent on a pooled event.  The fork / join edges between the step's main stream and its weight-gradient
 * stream (torch.cuda.Event record / wait in earlier rounds), as one plan-recordable C call.  (ddpm_plan_run does not come through
 * here: it gives the same guarantee by the cheapest means the recorded sequence allows, see resolve().) */
int ddpm_stream_order(void* waiter, void* signaller) {
    if (waiter == signaller) return DDPM_OK;
    EventRing* r = ring_of_device();
    if (!r) return DDPM_ERR_LAUNCH;
    return record_and_wait(*r, (hipStream_t)waiter, (hipStream_t)signaller);
}

/* bytes of zero at p, stream-ordered (torch.zeros / Tensor.zero_ of the gradient staging buffers, as a plan-recordable call) */
int ddpm_fill_zero(void* p, long long bytes, void* stream) {
    if (bytes < 0) return DDPM_ERR_SHAPE;
    if (bytes == 0) return DDPM_OK;
    if (!p) return DDPM_ERR_NULL;
    return hipMemsetAsync(p, 0, (size_t)bytes, (hipStream_t)stream) == hipSuccess ? DDPM_OK : DDPM_ERR_LAUNCH;
}

void* ddpm_plan_create(void) { return new Plan(); }

int ddpm_plan_destroy(void* plan) {
    delete static_cast<Plan*>(plan);
    return DDPM_OK;
}

/* Append one call.  `entry` = exported name; `words` = its arguments in declaration order, one 64-bit word each (pointers and 64-bit
 * integers as they are, int sign- or zero-extended, float as its IEEE-754 bits in the low half).  Returns the entry's index, or
 * -DDPM_ERR_SHAPE for an unknown name / wrong argument count, -DDPM_ERR_NULL for null arguments. */
int ddpm_plan_append(void* plan, const char* entry, const unsigned long long* words, int n_words) {
    if (!plan || !entry || (!words && n_words > 0)) return -DDPM_ERR_NULL;
    Plan* p = static_cast<Plan*>(plan);
    for (int i = 0; i < kNumEntryPoints; ++i) {
        if (std::strcmp(kEntryPoints[i].name, entry) != 0) continue;
        if (kEntryPoints[i].nargs != n_words || kEntryPoints[i].kind == EP_SIZING) return -DDPM_ERR_SHAPE;
        Entry e;
        e.thunk = kEntryPoints[i].thunk;
        e.first_word = (int)p->words.size();
        e.ep = i;
        p->words.insert(p->words.end(), words, words + n_words);
        p->entries.push_back(e);
        return (int)p->entries.size() - 1;
    }
    return -DDPM_ERR_SHAPE;
}

/* Close the segment being built; returns its index.  The host may do anything between two segments of a run (the data-parallel
 * step issues its RCCL all-reduces there). */
int ddpm_plan_cut(void* plan) {
    if (!plan) return -DDPM_ERR_NULL;
    Plan* p = static_cast<Plan*>(plan);
    p->segment_end.push_back((int)p->entries.size());
    return (int)p->segment_end.size() - 1;
}

int ddpm_plan_segments(void* plan) {
    if (!plan) return -DDPM_ERR_NULL;
    Plan* p = static_cast<Plan*>(plan);
    const int closed = (int)p->segment_end.size();
    const int last_end = closed ? p->segment_end.back() : 0;
    return closed + ((int)p->entries.size() > last_end ? 1 : 0);
}

int ddpm_plan_entries(void* plan) { return plan ? (int)static_cast<Plan*>(plan)->entries.size() : -DDPM_ERR_NULL; }

/* Issue every call of one segment, in recorded order, each on the stream it was recorded with.  Stops at the first call that fails and
 * returns its status code (ddpm_plan_failed_entry then names it); 0 = everything enqueued. */
int ddpm_plan_run(void* plan, int segment) {
    if (!plan) return DDPM_ERR_NULL;
    Plan* p = static_cast<Plan*>(plan);
    const int closed = (int)p->segment_end.size();
    if (segment < 0 || segment > closed) return DDPM_ERR_SHAPE;
    const int first = segment ? p->segment_end[segment - 1] : 0;
    const int last = segment < closed ? p->segment_end[segment] : (int)p->entries.size();
    if (p->resolved_entries != p->entries.size() || p->resolved_cuts != p->segment_end.size()) resolve(p);
    const word_t* words = p->words.data();
    const Entry* e = p->entries.data();
    EventRing* ring = nullptr;          // taken once per run, and only by a segment that has an edge (a plan without one never touches the runtime here)
    DdpmLaunchEdge& arm = g_ddpm_launch_edge;
    for (int i = first; i < last; ++i) {
        const word_t* w = words + e[i].first_word;
        int rc = DDPM_OK;
        if (e[i].mode == RUN) {
            rc = e[i].thunk(w);
        } else if (e[i].mode == SKIP) {
            continue;
        } else {
            if (!ring && !(ring = ring_of_device())) rc = DDPM_ERR_LAUNCH;
            else if (e[i].mode == PRODUCER) {
                arm.stream = (hipStream_t)(uintptr_t)w[kEntryPoints[e[i].ep].nargs - 1];
                arm.event = next_event(*ring);
                arm.attached = false;
                arm.armed = true;
                rc = e[i].thunk(w);
                arm.armed = false;
                p->bound[i] = arm.attached ? arm.event : nullptr;
            } else {
                const hipStream_t waiter = (hipStream_t)(uintptr_t)w[0], signaller = (hipStream_t)(uintptr_t)w[1];
                const hipEvent_t ev = e[i].mode == WAIT ? p->bound[e[i].producer] : nullptr;
                // (a producer that launched nothing this time — an empty tensor list — leaves no event: record one, as an eager call does)
                if (ev) rc = hipStreamWaitEvent(waiter, ev, 0) == hipSuccess ? DDPM_OK : DDPM_ERR_LAUNCH;
                else rc = record_and_wait(*ring, waiter, signaller);
            }
        }
        if (rc != DDPM_OK) {
            p->failed_index = i;
            p->failed_status = rc;
            return rc;
        }
    }
    return DDPM_OK;
}

/* name of the entry point the last failing ddpm_plan_run stopped at (NULL: none failed); *index receives its position in the plan */
const char* ddpm_plan_failed_entry(void* plan, int* index) {
    if (!plan) return nullptr;
    Plan* p = static_cast<Plan*>(plan);
    if (index) *index = p->failed_index;
    return p->failed_index < 0 ? nullptr : kEntryPoints[p->entries[p->failed_index].ep].name;
}

/* does the executor know this entry point, and with how many arguments?  (-1: unknown) */
int ddpm_plan_entry_arity(const char* entry) {
    if (!entry) return -1;
    for (int i = 0; i < kNumEntryPoints; ++i)
        if (std::strcmp(kEntryPoints[i].name, entry) == 0) return kEntryPoints[i].nargs;
    return -1;
}

}  // extern "C"
