// The outer loop of the full-batch NMF solvers (MU: nmf.hip, HALS: nmf_hals.hip) with its lagged stop test.
#pragma once
#include "nmf_impl.hpp"

namespace dcp {

// Where one iteration's normalisation kernel puts max|D - D_new|: *md is zero on entry and takes the max, *md_next is
// cleared for the next iteration, the last workgroup to arrive (ticket) stores the max into the pinned word *host.
template <class T>
struct NmfStopSlots {
    T* md;
    T* md_next;
    unsigned int* ticket;
    T* host;
};

// batch_mu.py:16-26 for a method given as a Step:
//   void layout(WsLayout&)    takes the method's own workspace items (run twice by ws_lay_out: sizing, then carving)
//   int  prepare(h)           loop-invariant work on h->stream (may synchronise)
//   int  iterate(h, Xc, Xn, Dc, Dn, slots)   enqueues one iteration from (Xc, Dc) into (Xn, Dn)
// Iteration `it` reads (x_{it-1}, D_{it-1}) from (Xc, Dc) and writes (x_it, D_it) to (Xn, Dn); its max|dD| lands in
// pinned host slot it&1, which holds a sentinel of -1 until then (max|dD| >= 0 or NaN).  The stop test of iteration
// it-1 (batch_mu.py:22) is evaluated AFTER iteration it has been enqueued, so the GPU never idles on the host; when
// it-1 turns out to have converged, iteration it is discarded: its inputs (Xc, Dc) are exactly the state the
// reference returns.  No event in the loop: the barrier packet of a hipEventRecord (system-scope release) cost ~6 us
// of idle GPU per iteration behind the normalisation.
// resid_trace != nullptr (parity/debug mode, synchronous): ||(Y - x_it D_it) o mask||_F of every iteration.
template <class T, class Step>
int nmf_lagged_loop(dcp_handle* h, Step& step, const T* Y, const T* mask, T* X, T* D, int64_t N, int64_t F, int64_t K,
                    T tol, int maxiter, int* it_out, T* last_maxdiff, T* resid_trace) {
    const bool want_resid = resid_trace != nullptr;
    const int resid_blocks = 1024;
    T* D2 = nullptr;                  // second D buffer
    T* X2 = nullptr;                  // second x buffer
    T* maxdiff_dev = nullptr;         // max|dD| of the two iterations in flight
    unsigned int* ticket = nullptr;   // arrival ticket of the normalisation's workgroups
    T* resid_tmp = nullptr;
    double* resid_part = nullptr;
    DCP_TRY(ws_lay_out(h, [&](WsLayout& a) {
        step.layout(a);
        a.take(D2, (size_t)K * F);
        a.take(X2, (size_t)N * K);
        a.take(maxdiff_dev, 2);
        a.take(ticket, 4);
        if (want_resid) {
            a.take(resid_tmp, (size_t)N * F);
            a.take(resid_part, resid_blocks);
        }
    }));
    void* hostv = nullptr;
    DCP_TRY(host_scratch(h, sizeof(double) * (resid_blocks + 4), &hostv));
    T* host_md = reinterpret_cast<T*>(hostv);             // [2]
    double* host_part = reinterpret_cast<double*>(hostv) + 2;

    DCP_TRY(step.prepare(h));
    DCP_HIP_OK(h, hipMemsetAsync(maxdiff_dev, 0, 2 * sizeof(T), h->stream));
    DCP_HIP_OK(h, hipMemsetAsync(ticket, 0, 4 * sizeof(unsigned int), h->stream));

    T* Xc = X;  T* Xn = X2;
    T* Dc = D;  T* Dn = D2;
    int result_it = maxiter;   // batch_mu.py:26
    T md_last = T(0);
    bool converged = false;
    for (int it = 1; it < maxiter; ++it) {  // batch_mu.py:16
        const int slot = it & 1;
        // the host consumed this slot's previous value during iteration it-1; nothing that stores into it is enqueued
        *reinterpret_cast<volatile T*>(host_md + slot) = T(-1);
        DCP_TRY(step.iterate(h, Xc, Xn, Dc, Dn,
                             NmfStopSlots<T>{maxdiff_dev + slot, maxdiff_dev + (slot ^ 1), ticket, host_md + slot}));
        if (want_resid) {
            double acc = 0.0;
            DCP_TRY(nmf_residual<T>(h, Y, mask, Xn, Dn, N, F, K, resid_tmp, resid_part, resid_blocks));
            DCP_TRY(read_partial_sum(h, resid_part, resid_blocks, host_part, &acc));
            resid_trace[it - 1] = (T)sqrt(acc);
        }
        if (it > 1) {   // stop test of the PREVIOUS iteration
            DCP_TRY(wait_pinned_word(h, host_md + (slot ^ 1), T(-1), &md_last));
            if (md_last < tol) {   // a NaN compares false, as in NumPy
                result_it = it - 1;
                converged = true;
                break;             // (Xc, Dc) hold x_{it-1} and D_new of iteration it-1
            }
        }
        T* t = Xc; Xc = Xn; Xn = t;
        t = Dc; Dc = Dn; Dn = t;
    }
    if (!converged && maxiter > 1) {   // stop test of the last iteration
        const int slot = (maxiter - 1) & 1;
        DCP_TRY(wait_pinned_word(h, host_md + slot, T(-1), &md_last));
        if (md_last < tol) result_it = maxiter - 1;
    }
    DCP_HIP_OK(h, hipStreamSynchronize(h->stream));   // drain (incl. a discarded iteration)
    if (Xc != X)
        DCP_HIP_OK(h, hipMemcpyAsync(X, Xc, sizeof(T) * (size_t)N * K, hipMemcpyDeviceToDevice, h->stream));
    if (Dc != D)
        DCP_HIP_OK(h, hipMemcpyAsync(D, Dc, sizeof(T) * (size_t)K * F, hipMemcpyDeviceToDevice, h->stream));
    DCP_HIP_OK(h, hipStreamSynchronize(h->stream));
    *it_out = result_it;
    if (last_maxdiff) *last_maxdiff = md_last;
    return DCP_OK;
}

}  // namespace dcp
