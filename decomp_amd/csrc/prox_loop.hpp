// The outer loop of the proximal-gradient LASSO solvers (ista / acc_ista / fista; dense: lasso_impl.hpp, structured:
// template_impl.hpp) with its lagged stop test, and the stop flag's way to the host.
#pragma once
#include <math.h>

#include "handle.hpp"
#include "scalar.hpp"

namespace dcp {

// *host = *flag, *flag = 0: the stop flag of a check iteration goes to device-mapped pinned host memory (the host polls
// it one iteration later) and is cleared for the next check.  One 2 us launch instead of a fill kernel in front of the
// iteration, a copy kernel behind it and an event (whose barrier packet idles the GPU ~5 us): 14 -> ~3 us per check.
template <class T = void>
__global__ void flag_publish_kernel(int* __restrict__ flag, int* __restrict__ host) {
    if (threadIdx.x == 0) {
        const int f = *flag;
        *flag = 0;
        *host = f;
    }
}

// Wait for flag_publish_kernel's store: the word was set to the sentinel -1 before that kernel was enqueued (polling:
// the GPU sat idle ~2 ms per dictionary step behind a blocking wait once the host ran a step ahead).
inline int poll_host_flag(dcp_handle* h, int* host_flag) { return wait_pinned_word(h, host_flag, -1); }

template <class T>
struct ProxLoopResult {
    int it;           // the reference's iteration count
    T* result;        // the buffer that holds the returned iterate
    bool converged;   // a stop test was met (the iteration enqueued behind it, if any, was discarded)
};

// lasso.py:283-297 (ista), :343-357 (acc_ista), :401-415 (fista) from the iterate in xb[0], for a solver given as
//   int step(i, V, P, Nw, Vn, coef, check, is_last)   enqueues iteration i on h->stream
// Buffer roles (the pointers rotate over the four buffers xb):
//   P = the iterate the stop test compares with (the reference's x0)
//   V = the point fed to the step (x0 for ista, v / w0 with momentum)
//   Nw, Vn = this iteration's outputs (x0_new and the next V; Vn is null for ista)
// coef is the momentum coefficient; check != 0 asks the step to raise *flag when its stop test is violated (*flag is
// zero on entry: the caller's prepare kernels, flag_publish_kernel afterwards).
// The stop test of a check iteration (i % 10 == 0, lasso.py:293) is read ONE iteration late: its flag travels to the
// host (flag_publish_kernel) while iteration i + 1 is already enqueued, so the GPU does not idle through a host round
// trip in the middle of every solve (the dictionary step runs ten iterations and checks at i = 0).  Iteration i + 1
// only READS iteration i's output, so when the test had passed that output is still intact and i + 1 is simply
// discarded.
template <class T, class Step>
inline int prox_gradient_loop(dcp_handle* h, T* const* xb, int method, int maxiter, int* flag, int* host_flag,
                              Step&& step, ProxLoopResult<T>* out) {
    typedef real_t<T> R;
    const bool mom = (method != DCP_LASSO_ISTA);
    T* P = xb[0];
    T* V = xb[0];
    T* lastP = xb[0];      // P of the last completed iteration (whose output is P by now)
    double beta = 1.0;
    *out = ProxLoopResult<T>{maxiter - 1, xb[0], false};
    int pend_i = -1;       // the check iteration whose flag is on its way, and its output
    T* pend_x = nullptr;
    auto resolve = [&]() -> int {
        DCP_TRY(poll_host_flag(h, host_flag));
        if (*host_flag == 0) *out = ProxLoopResult<T>{pend_i, pend_x, true};   // lasso.py:293-294
        pend_i = -1;
        return DCP_OK;
    };
    for (int i = 0; i < maxiter; ++i) {
        T* Nw = nullptr;
        T* Vn = nullptr;
        for (int b = 0; b < 4; ++b) {
            T* c = xb[b];
            if (c == P || c == V) continue;
            if (Nw == nullptr) Nw = c;
            else if (Vn == nullptr) Vn = c;
        }
        R coef = R(0);
        double beta_new = beta;
        if (method == DCP_LASSO_ACC_ISTA) {
            coef = (R)((double)i / (double)(i + 3));                    // lasso.py:353
        } else if (method == DCP_LASSO_FISTA) {
            beta_new = 0.5 * (1.0 + sqrt(1.0 + 4.0 * beta * beta));     // lasso.py:411
            coef = (R)((beta - 1.0) / beta_new);
        }
        const int check = (i % 10 == 0) ? 1 : 0;
        DCP_TRY(step(i, V, P, Nw, mom ? Vn : (T*)nullptr, coef, check, i == maxiter - 1));
        if (pend_i >= 0) {   // the check iteration before this one: was its test met?
            DCP_TRY(resolve());
            if (out->converged) return DCP_OK;   // this iteration is discarded
        }
        if (check) {
            *reinterpret_cast<volatile int*>(host_flag) = -1;   // sentinel: nothing is in flight into it here
            hipLaunchKernelGGL(flag_publish_kernel<void>, dim3(1), dim3(64), 0, h->stream, flag, host_flag);
            DCP_LAUNCH_OK(h, hipGetLastError());
            pend_i = i;
            pend_x = Nw;
        }
        lastP = P;
        P = Nw;
        V = mom ? Vn : Nw;
        beta = beta_new;
    }
    if (pend_i >= 0) DCP_TRY(resolve());   // a check on the very last iteration
    // QUIRK: on exhaustion ista / fista return the latest iterate, acc_ista the one
    // before it (its `x0 = x0_new` sits at the top of the loop body, lasso.py:351-357).
    if (!out->converged) out->result = (method == DCP_LASSO_ACC_ISTA) ? lastP : P;
    return DCP_OK;
}

}  // namespace dcp
