// Opaque library handle: device binding, stream, grow-only device workspace and
// pinned host scalars for read-backs.  One handle per process/device; calls on one
// handle are not re-entrant.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>

#include "../../include/decomp_hip.h"
#include "scalar.hpp"

struct dcp_handle {
    int device = 0;
    hipStream_t stream = nullptr;
    // The workspace arena is shared by every arena-using call on this handle.  arena_stream is the stream
    // the last such call enqueued on; when the next one runs on a different stream (dcp_set_stream in
    // between), ws_reserve makes the new stream wait for the old one with this event -- calls that never
    // touch the arena (the row movers of the out-of-core feed) are not ordered against anything.
    hipEvent_t stream_switch = nullptr;
    hipStream_t arena_stream = nullptr;
    bool arena_stream_set = false;
    // Side stream for work that can run BESIDE a kernel that leaves most of the chip idle (the atom
    // sweep's look-ahead product next to the one-workgroup recursion); created on first use and
    // ordered against the main stream with events only (side_after_main / main_after_side).
    hipStream_t side = nullptr;
    hipEvent_t ev_main = nullptr, ev_side = nullptr;
    // Workspace: one grow-only arena.  A public call describes its buffers once (ws_lay_out): the description is
    // walked to size the total, the total is reserved (ws_reserve: reallocates only when it outgrows the arena,
    // i.e. on the first call of a given problem size, never in steady state), and walked again to hand them out.
    char* arena = nullptr;
    size_t arena_bytes = 0;
    size_t arena_used = 0;
    // pinned host scratch for scalar read-backs
    void* host_pinned = nullptr;
    size_t host_pinned_bytes = 0;
    std::string err;
    // RCCL communicator of the sample-sharded solvers (comm.hip; ncclComm_t kept opaque here)
    void* comm = nullptr;
    int comm_rank = 0, comm_world = 1;
    // ... or a caller-supplied exchange (dcp_comm_set_external: MPI, gloo, a test double)
    dcp_allreduce_fn comm_ext = nullptr;
    void* comm_ext_user = nullptr;
    // a row gather registered by dcp_dict_prefetch_rows_bytes: the next dictionary step runs it on the side
    // stream beside its atom sweep (rows of the NEXT minibatch while the chip is nearly idle)
    const void* pf_in = nullptr;
    const int64_t* pf_index = nullptr;
    void* pf_out = nullptr;
    int64_t pf_rows = 0, pf_row_bytes = 0;
    bool pf_inflight = false;   // started on the side stream, not yet joined
    // coordinate descent inside the dictionary step: the stop flag of the solve's last ten sweeps is still on its way
    // to this pinned word when lasso_cd_gram, which arms the deferral, returns; lasso_settle_deferred() turns it into
    // *lasso_deferred_it
    int* lasso_deferred_flag = nullptr;
    int* lasso_deferred_it = nullptr;
    int lasso_deferred_it_met = 0;
    bool lasso_deferred_copy = false;   // the pinned word holds the count itself (orthogonal matching pursuit)
    int lasso_it_sink = 0;
    // parallel_cd inside the dictionary step: the caller-supplied shuffle table (dcp_dict_set_pcd_order)
    const int* pcd_order = nullptr;
    int64_t pcd_rows = 0, pcd_K = 0;
    // optional per-kernel timing (dcp_profile_*): hipEvent pairs around labelled launches
    bool prof_on = false;
    unsigned prof_mask = 0xffffffffu;   // labels that are timed while prof_on
    struct ProfRec { int label; hipEvent_t a, b; };
    std::vector<ProfRec> prof_recs;
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[DCP_PROF_NLABELS] = {0};
    long long prof_cnt[DCP_PROF_NLABELS] = {0};
    // float32 products of the NMF Gram path (dcp_set_f32_product_mode): 0 = split-bf16 core (bf16x6,
    // gemm_mfma_bf16x6.hpp), 1 = the exact fp32 MFMA core
    int f32_product_mode = 0;
    // beta of DCP_LIK_BETA (dcp_set_nmf_beta), read when an NMF call that passes DCP_LIK_BETA is enqueued
    double nmf_beta = 0.0;
    // L1 / L2 penalty on the NMF codes (dcp_set_nmf_penalty), read when an MU or HALS loop or split step is
    // enqueued; every other entry ignores it
    double nmf_l1 = 0.0, nmf_l2 = 0.0;
};

namespace dcp {

inline int fail(dcp_handle* h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

#define DCP_HIP_OK(h, expr)                                                                  \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return dcp::fail((h), DCP_ERR_HIP,                                               \
                             std::string(#expr) + ": " + hipGetErrorString(_e));             \
    } while (0)

// the status of a kernel launch (hipGetLastError() after it, or what a launcher returned)
#define DCP_LAUNCH_OK(h, what)                                                        \
    do {                                                                              \
        hipError_t _e = (what);                                                       \
        if (_e != hipSuccess)                                                         \
            return dcp::fail((h), DCP_ERR_HIP, std::string("launch failed: ") +       \
                                                   hipGetErrorString(_e));            \
    } while (0)

#define DCP_TRY(expr)                  \
    do {                               \
        int _rc = (expr);              \
        if (_rc != DCP_OK) return _rc; \
    } while (0)

// Times everything enqueued on the handle's stream during its lifetime under `label`
// (only when profiling is on; otherwise free).
struct ProfScope {
    dcp_handle* h;
    int label;
    hipEvent_t a = nullptr, b = nullptr;
    static hipEvent_t take(dcp_handle* h) {
        if (!h->prof_pool.empty()) {
            hipEvent_t e = h->prof_pool.back();
            h->prof_pool.pop_back();
            return e;
        }
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) return nullptr;
        return e;
    }
    ProfScope(dcp_handle* h_, int label_) : h(h_), label(label_) {
        if (!h->prof_on || !((h->prof_mask >> label) & 1u)) return;
        a = take(h);
        b = take(h);
        if (a) (void)hipEventRecord(a, h->stream);
    }
    ~ProfScope() {
        if (!a || !b) return;
        (void)hipEventRecord(b, h->stream);
        h->prof_recs.push_back({label, a, b});
    }
};

// Events that only order the handle's two streams on ONE device: no timing, and no system-scope fence when they are
// recorded (the default's cache write-back idles the recording stream ~6 us; nothing on the host reads behind them).
constexpr unsigned kOrderingEvent = hipEventDisableTiming | hipEventDisableSystemFence;

// what is enqueued on h->side after this call starts after the work already on h->stream
inline int side_after_main(dcp_handle* h) {
    if (h->side == nullptr) {
        if (hipStreamCreateWithFlags(&h->side, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_main, kOrderingEvent) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_side, kOrderingEvent) != hipSuccess)
            return fail(h, DCP_ERR_HIP, "side stream creation failed");
    }
    if (hipEventRecord(h->ev_main, h->stream) != hipSuccess ||
        hipStreamWaitEvent(h->side, h->ev_main, 0) != hipSuccess)
        return fail(h, DCP_ERR_HIP, "side stream fork failed");
    return DCP_OK;
}
// what is enqueued on h->stream after this call starts after the work already on h->side
inline int main_after_side(dcp_handle* h) {
    if (hipEventRecord(h->ev_side, h->side) != hipSuccess ||
        hipStreamWaitEvent(h->stream, h->ev_side, 0) != hipSuccess)
        return fail(h, DCP_ERR_HIP, "side stream join failed");
    return DCP_OK;
}

// gather / scatter rows on `stream` (util.hip; the row movers of the minibatch containers)
int move_rows_on(dcp_handle* h, hipStream_t stream, const void* in, const int64_t* in_index, void* out,
                 const int64_t* out_index, int64_t rows, int64_t row_bytes);

// Starts the handle's registered row gather on the side stream, ordered after what is on the main stream now.
inline int start_registered_prefetch(dcp_handle* h) {
    if (h->pf_rows <= 0 || h->pf_row_bytes <= 0) return DCP_OK;
    DCP_TRY(side_after_main(h));
    DCP_TRY(move_rows_on(h, h->side, h->pf_in, h->pf_index, h->pf_out, nullptr, h->pf_rows, h->pf_row_bytes));
    h->pf_rows = 0;
    h->pf_inflight = true;
    return DCP_OK;
}

// The arena's previous user may still be running on another stream: the current stream waits for it
// (an event recorded on the previous stream, no host sync).  decomp_hip.h makes the caller keep that stream
// alive until this point; the device synchronisation below only covers a FAILED record / wait on a live
// stream (it is not a defence against a destroyed one: that is a use-after-free inside the runtime).
inline void ws_order_streams(dcp_handle* h) {
    if (h->arena_stream_set && h->arena_stream != h->stream && h->arena != nullptr) {
        bool ok = false;
        if (h->stream_switch == nullptr)
            (void)hipEventCreateWithFlags(&h->stream_switch, kOrderingEvent);
        if (h->stream_switch != nullptr && hipEventRecord(h->stream_switch, h->arena_stream) == hipSuccess &&
            hipStreamWaitEvent(h->stream, h->stream_switch, 0) == hipSuccess)
            ok = true;
        if (!ok) {
            (void)hipGetLastError();
            (void)hipDeviceSynchronize();
        }
    }
    h->arena_stream = h->stream;
    h->arena_stream_set = true;
}

// Reserve the total workspace for a call up front (so no allocation happens
// between kernels).  Returns DCP_OK or an error code.  Every arena-using entry point calls this first.
inline int ws_reserve(dcp_handle* h, size_t bytes) {
    ws_order_streams(h);
    if (bytes <= h->arena_bytes) return DCP_OK;
    if (h->arena) {
        hipError_t e = hipStreamSynchronize(h->stream);
        if (e != hipSuccess) return fail(h, DCP_ERR_HIP, hipGetErrorString(e));
        (void)hipFree(h->arena);
        h->arena = nullptr;
        h->arena_bytes = 0;
    }
    size_t want = bytes + (bytes >> 3) + (1u << 20);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, want);
    if (e != hipSuccess) {
        want = bytes;
        e = hipMalloc(&p, want);
    }
    if (e != hipSuccess)
        return fail(h, DCP_ERR_NOMEM,
                    "workspace hipMalloc of " + std::to_string(bytes) + " bytes failed: " +
                        hipGetErrorString(e));
    h->arena = static_cast<char*>(p);
    h->arena_bytes = want;
    h->arena_used = 0;
    return DCP_OK;
}

inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

// One walk over a call's workspace items.  Without a base it only adds up the sizes (every pointer comes back null);
// based at the arena it hands out the same items in the same order, each 256-byte aligned.
struct WsLayout {
    char* base = nullptr;
    size_t used = 0;
    template <class T>
    void take(T*& p, size_t count) {
        p = base ? reinterpret_cast<T*>(base + used) : nullptr;
        used += align256(count * sizeof(T));
    }
};

// Sizes, reserves and hands out a call's whole workspace from ONE description: `items(WsLayout&)` runs twice, first
// to size the reservation, then based at the arena.  It may only call take() and set fields derived from the sizes
// (slab_count): it must not read the pointers, touch the handle or enqueue anything.  A workspace struct has one
// layout function (lasso_layout, atom_layout, ...) that entry points compose inside `items`.
template <class Items>
inline int ws_lay_out(dcp_handle* h, Items&& items) {
    WsLayout sizing;
    items(sizing);
    DCP_TRY(ws_reserve(h, sizing.used));
    WsLayout carving{h->arena};
    items(carving);
    h->arena_used = carving.used;
    if (carving.used != sizing.used)
        return fail(h, DCP_ERR_INTERNAL, "workspace plan mismatch: the sizing walk and the carving walk differ");
    return DCP_OK;
}

inline int host_scratch(dcp_handle* h, size_t bytes, void** out) {
    if (bytes > h->host_pinned_bytes) {
        if (h->host_pinned) (void)hipHostFree(h->host_pinned);
        h->host_pinned = nullptr;
        h->host_pinned_bytes = 0;
        size_t want = bytes < 4096 ? 4096 : bytes;
        hipError_t e = hipHostMalloc(&h->host_pinned, want, hipHostMallocDefault);
        if (e != hipSuccess) return fail(h, DCP_ERR_NOMEM, "hipHostMalloc failed");
        h->host_pinned_bytes = want;
    }
    *out = h->host_pinned;
    return DCP_OK;
}

// Waits until a kernel on h->stream has stored over the `sentinel` the host put into a pinned (device-mapped) word
// before that kernel was enqueued; *out (if given) is the word then.  Polling instead of sleeping in a blocking wait,
// which wakes up late; a stream synchronisation is the fallback after ~2 s.  A NaN counts as stored.
template <class W>
inline int wait_pinned_word(dcp_handle* h, const W* word, W sentinel, W* out = nullptr) {
    const volatile W* v = word;
    for (long spin = 0; *v == sentinel; ++spin) {
        if (spin == 400000000L) {
            DCP_HIP_OK(h, hipStreamSynchronize(h->stream));
            break;
        }
        __builtin_ia32_pause();
    }
    if (out) *out = *v;
    return DCP_OK;
}

// pinned[0 .. n) <- dev[0 .. n) once h->stream has run: one copy on the stream, one stream synchronisation
template <class W>
inline int read_words(dcp_handle* h, const W* dev, int n, W* pinned) {
    DCP_HIP_OK(h, hipMemcpyAsync(pinned, dev, sizeof(W) * n, hipMemcpyDeviceToHost, h->stream));
    DCP_HIP_OK(h, hipStreamSynchronize(h->stream));
    return DCP_OK;
}

// *out <- the device scalar *dev through `pinned`, or through the start of the handle's pinned scratch
template <class W, class O>
inline int read_scalar(dcp_handle* h, const W* dev, O* out, W* pinned = nullptr) {
    void* hostv = pinned;
    if (pinned == nullptr) DCP_TRY(host_scratch(h, 64, &hostv));
    DCP_TRY(read_words(h, dev, 1, static_cast<W*>(hostv)));
    *out = (O)*static_cast<W*>(hostv);
    return DCP_OK;
}

// Sum / maximum (NaN wins, as np.max) of n doubles in device memory -- per-workgroup partials, taken in order --
// through `pinned`
inline int read_partial_sum(dcp_handle* h, const double* part_dev, int n, double* pinned, double* sum) {
    DCP_TRY(read_words(h, part_dev, n, pinned));
    double acc = 0.0;
    for (int i = 0; i < n; ++i) acc += pinned[i];
    *sum = acc;
    return DCP_OK;
}
inline int read_partial_max(dcp_handle* h, const double* part_dev, int n, double* pinned, double* max) {
    DCP_TRY(read_words(h, part_dev, n, pinned));
    double m = 0.0;
    for (int i = 0; i < n; ++i) m = max_np(pinned[i], m);
    *max = m;
    return DCP_OK;
}

}  // namespace dcp
