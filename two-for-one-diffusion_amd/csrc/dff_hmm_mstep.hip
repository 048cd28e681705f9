// dff_hmm_mstep.hip -- the control word and the M-step of Baum-Welch on the device (dff_hmm_fit_steps): one launch of ONE
// workgroup after every E-step of dff_hmm.hip, so that many iterations run back to back without a host read.
//
// dff_hmm_fit_mstep_kernel   reads the E-step's packed statistics (loglik | xi (m, m) | gamma0 (m) | gamma_sym (m, K)) and its status
//     word from the workspace and the fit's state word, and decides: a stopped fit writes a NaN log-likelihood and nothing
//     else; a failed E-step stops the fit (2); a log-likelihood within `accuracy` of the last one stops it (1) with the
//     parameters it was computed with; otherwise the parameters are re-estimated IN PLACE, in fp64, every sum in index order
//     from +0, one term after the other:
//       waves 1 .. 3   p0' = gamma0 / sum(gamma0); B'[i, :] = Gamma[i, :] / occ_i, one wave per row at a time: the lanes fetch 64
//                      consecutive terms, then every lane adds all 64 in index order (hmm_lane of dff_hmm.hip);
//       wave 0         A.  Lane 8 i + j holds the pair (i, j).  Not reversible: A'_ij = Xi_ij / r_i.  Reversible: the graph of the
//                      pairs with Xi_ij > 0 is one 64-bit ballot, its strong connectivity two closures of bit masks from state
//                      0 (forward and backward); then the fixed-point sweeps of the reversible estimator in registers --
//                      S_ij = Xi_ij + Xi_ji, c_i = sum_j Xi_ij, x_i = sum_j S_ij / 2; per sweep q_i = c_i / x_i, t_ij = S_ij / (q_i + q_j)
//                      (+0 where S_ij = 0), x_i' = sum_j t_ij, err = max_i |x_i' - x_i| / x_i -- q_j and the t_ij of a row travel by
//                      __shfl (the wave's permute network: no LDS traffic, no barrier), the stopping rule is two ballots.  Every
//                      lane of row i carries x_i, computed by the same instructions on the same values.
//     No expression multiplies before it adds (x / 2 is exact), and contraction is off: the bits are those of the numpy
//     statement tests/hmm_fit_cases.py makes.  A row whose occupancy is not positive keeps its values (flag bit 0); a
//     reversible step on a graph that is not strongly connected stops the fit (3) and changes no parameter.
#pragma once
#include "../../include/dff.h"   // dff_hmm_fit_state
#include "dff_hmm.hip"

#define DFF_HMM_FIT_THREADS 256

// S_ij / (q_i + q_j), +0 where the pair has no counts
__device__ __forceinline__ double hmm_fit_flow(double S, double qi, double qj) { return S != 0.0 ? S / (qi + qj) : 0.0; }

// the sweeps of wave 0: x (this lane's row) is advanced in place -> the sweeps spent; capped: they ran out before err < tol
template <int M>
__device__ __forceinline__ long long hmm_fit_sweeps(double S, double c, double& x, bool act, int lane, double tol,
                                                    long long max_sweeps, bool& capped) {
#pragma clang fp contract(off)
    const int j = lane & 7, row = lane & ~7;
    long long n = 0;
    bool met = false;
    while (n < max_sweeps) {
        const double q = c / x;
        const double qj = __shfl(q, j << 3);
        const double t = act ? hmm_fit_flow(S, q, qj) : 0.0;
        double xn = 0.0;
#pragma unroll
        for (int jj = 0; jj < M; ++jj) xn += __shfl(t, row | jj);
        const double e = fabs(xn - x) / x;
        x = xn;
        ++n;
        // err = max_i e_i: below tol when every e_i is; not finite when one e_i is not (no e_i is negative: S, c >= 0)
        const unsigned long long small = __ballot(!act || e < tol);
        const unsigned long long wild = __ballot(act && !(fabs(e) < __builtin_inf()));
        if (small == ~0ull) { met = true; break; }
        if (wild) break;
    }
    capped = !met && n >= max_sweeps;
    return n;
}

// the reversible estimator of wave 0 on m >= 2 strongly connected states: A, pi and the sweeps spent
template <int M>
__device__ __forceinline__ long long hmm_fit_reversible(const double* __restrict__ xi, double xij, double xji, bool act, int lane,
                                                        double tol, long long max_sweeps, double* __restrict__ trans,
                                                        double* __restrict__ stationary, bool& capped) {
#pragma clang fp contract(off)
    const int i = lane >> 3, j = lane & 7, row = lane & ~7;
    const double S = act ? xij + xji : 0.0;
    double c = 0.0, x = 0.0;
#pragma unroll
    for (int jj = 0; jj < M; ++jj) {
        c += i < M ? xi[i * M + jj] : 0.0;
        x += __shfl(S, row | jj);
    }
    x = 0.5 * x;
    const long long n = hmm_fit_sweeps<M>(S, c, x, act, lane, tol, max_sweeps, capped);
    const double q = c / x;
    const double qj = __shfl(q, j << 3);
    const double flow = act ? hmm_fit_flow(S, q, qj) : 0.0;
    double sx = 0.0;
#pragma unroll
    for (int ii = 0; ii < M; ++ii) sx += __shfl(x, ii << 3);
    if (act) trans[i * M + j] = flow / x;
    if (stationary && act && j == 0) stationary[i] = x / sx;
    return n;
}

__global__ __launch_bounds__(DFF_HMM_FIT_THREADS) void dff_hmm_fit_mstep_kernel(const double* __restrict__ stats,
                                                                                const int* __restrict__ status,
                                                                                dff_hmm_fit_state* __restrict__ state,
                                                                                double* __restrict__ trans, double* __restrict__ emit,
                                                                                double* __restrict__ init, int m, int K, int reversible,
                                                                                double accuracy, double rev_tol, long long rev_max_sweeps,
                                                                                double* __restrict__ loglik_out,
                                                                                double* __restrict__ stationary) {
#pragma clang fp contract(off)
    __shared__ int sh_flags;
    __shared__ long long sh_sweeps;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const dff_hmm_fit_state st = *state;                            // every thread reads the same words ...
    const int est = *status;
    const double L = stats[0];
    if (tid == 0) { sh_flags = 0; sh_sweeps = 0; }
    __syncthreads();                                                // ... before thread 0 rewrites them
    const double nan = __builtin_nan("");
    if (st.stop != 0) {                                             // a stopped fit: nothing changes
        if (tid == 0) *loglik_out = nan;
        return;
    }
    const int n_estep = st.n_estep + 1;
    if (est != 0) {                                                 // the E-step failed
        if (tid == 0) {
            state->n_estep = n_estep;
            state->estep_status = est;
            state->stop = 2;
            *loglik_out = nan;
        }
        return;
    }
    if (n_estep > 1 && fabs(L - st.last_loglik) < accuracy) {       // converged: the parameters stay those L was computed with
        if (tid == 0) {
            state->n_estep = n_estep;
            state->estep_status = 0;
            state->stop = 1;
            state->last_loglik = L;
            *loglik_out = L;
        }
        return;
    }
    const double* xi = stats + 1;
    const double* g0 = xi + m * m;
    const double* gs = g0 + m;
    const int i = lane >> 3, j = lane & 7;
    const bool act = i < m && j < m;
    const double xij = act ? xi[i * m + j] : 0.0, xji = act ? xi[j * m + i] : 0.0;
    // strongly connected over all m states: everything is reached from state 0 and reaches it
    bool go = true;
    if (reversible && m > 1) {
        const unsigned long long adj = __ballot(act && xij > 0.0);  // bit 8 i + j: an edge i -> j
        unsigned fwd = 1u, bwd = 1u;
        for (int it = 0; it < m; ++it)
            for (int a = 0; a < m; ++a) {
                const unsigned out = (unsigned)(adj >> (8 * a)) & 0xFFu;
                if ((fwd >> a) & 1u) fwd |= out;
                if (out & bwd) bwd |= 1u << a;
            }
        const unsigned all = (1u << m) - 1u;
        go = fwd == all && bwd == all;
    }
    if (wave == 0) {
        if (!go) {
        } else if (reversible) {
            long long n = 0;
            bool capped = false;
            switch (m) {
                case 1:
                    if (lane == 0) { trans[0] = 1.0; if (stationary) stationary[0] = 1.0; }
                    break;
                case 2: n = hmm_fit_reversible<2>(xi, xij, xji, act, lane, rev_tol, rev_max_sweeps, trans, stationary, capped); break;
                case 3: n = hmm_fit_reversible<3>(xi, xij, xji, act, lane, rev_tol, rev_max_sweeps, trans, stationary, capped); break;
                case 4: n = hmm_fit_reversible<4>(xi, xij, xji, act, lane, rev_tol, rev_max_sweeps, trans, stationary, capped); break;
                case 5: n = hmm_fit_reversible<5>(xi, xij, xji, act, lane, rev_tol, rev_max_sweeps, trans, stationary, capped); break;
                case 6: n = hmm_fit_reversible<6>(xi, xij, xji, act, lane, rev_tol, rev_max_sweeps, trans, stationary, capped); break;
                case 7: n = hmm_fit_reversible<7>(xi, xij, xji, act, lane, rev_tol, rev_max_sweeps, trans, stationary, capped); break;
                default: n = hmm_fit_reversible<8>(xi, xij, xji, act, lane, rev_tol, rev_max_sweeps, trans, stationary, capped); break;
            }
            if (lane == 0) {
                sh_sweeps = n;
                if (capped) atomicOr(&sh_flags, 2);
            }
        } else {
            double r = 0.0;
            for (int jj = 0; jj < m; ++jj) r += i < m ? xi[i * m + jj] : 0.0;
            if (act) {
                if (r > 0.0) trans[i * m + j] = xij / r;
                else atomicOr(&sh_flags, 1);
            }
        }
    } else {
        if (wave == 1 && lane < m) {
            double g = 0.0;
            for (int ii = 0; ii < m; ++ii) g += g0[ii];
            if (g > 0.0 && go) init[lane] = g0[lane] / g;
        }
        for (int r = wave - 1; r < m; r += DFF_HMM_FIT_THREADS / 64 - 1) {
            const double* row = gs + (size_t)r * K;
            double occ = 0.0;
            for (int base = 0; base < K; base += 64) {
                const double v = base + lane < K ? row[base + lane] : 0.0;
#pragma unroll
                for (int l = 0; l < 64; ++l) occ += hmm_lane(v, l);
            }
            if (occ > 0.0) {
                if (go)
                    for (int s = lane; s < K; s += 64) emit[(size_t)r * K + s] = row[s] / occ;
            } else if (lane == 0) {
                atomicOr(&sh_flags, 1);
            }
        }
    }
    __syncthreads();
    if (tid == 0) {
        state->n_estep = n_estep;
        state->estep_status = 0;
        state->stop = go ? 0 : 3;
        state->flags = st.flags | sh_flags;
        state->last_loglik = L;
        state->rev_sweeps = st.rev_sweeps + sh_sweeps;
        *loglik_out = L;
    }
}
