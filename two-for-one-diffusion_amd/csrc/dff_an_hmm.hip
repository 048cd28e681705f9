// dff_an_hmm.hip -- the hidden-Markov-model entry points of include/dff.h and the kernels they launch: dff_hmm_plan,
// dff_hmm_estep, dff_hmm_fit_steps, dff_hmm_viterbi with their workspace functions and stage knobs.  One of four analysis
// units (dff_analysis_host.h names them).
#include "dff_analysis_host.h"

#include "dff_hmm.hip"
#include "dff_hmm_viterbi.hip"
#include "dff_hmm_mstep.hip"

// ---------------------------------------------------------------------------------------------
// Hidden Markov models: one E-step of Baum-Welch over all chains (dff_hmm.hip)
// ---------------------------------------------------------------------------------------------
extern "C" int dff_hmm_chunk(void) { return DFF_HMM_CHUNK; }

// how many of the call's launches run: 0 = all of them; 1 .. 5 = stop after the parameters, the chunk products, the carries, the
// apply pass, the emission counts (benchmarks: the share of every launch, by differences; the outputs are then unfinished)
static std::atomic<int> g_hmm_stages{0};

extern "C" int dff_debug_hmm_stages(int stages) {
    if (stages < 0 || stages > 5) return fail(DFF_EINVAL, "debug_hmm_stages: 0 (all) or 1 .. 5 launches");
    g_hmm_stages.store(stages);
    return DFF_OK;
}

// chains and chunks of a call, and (cpre != null) the chunks before every trajectory: cpre[0 .. n_traj]
static int hmm_plan(const long long* lengths, int n_traj, int lag, long long* n_chains, long long* n_chunks, long long* cpre,
                    const char* what) {
    if (lag < 1) return fail(DFF_EINVAL, "%s: lag must be >= 1", what);
    if (n_traj < 0 || (n_traj > 0 && !lengths)) return fail(DFF_EINVAL, "%s: null / negative trajectory lengths", what);
    if ((long long)n_traj * lag > DFF_HMM_MAXCHAINS)
        return fail(DFF_EINVAL, "%s: %lld chains, at most %d", what, (long long)n_traj * lag, DFF_HMM_MAXCHAINS);
    long long chunks = 0;
    for (int r = 0; r < n_traj; ++r) {
        if (lengths[r] < 0) return fail(DFF_EINVAL, "%s: trajectory %d has negative length", what, r);
        if (cpre) cpre[r] = chunks;
        const auto [q, rem] = hmm_split(lengths[r], lag);
        chunks += rem * hmm_chunks_of(q + 1) + (lag - rem) * hmm_chunks_of(q);
    }
    if (cpre) cpre[n_traj] = chunks;
    if (n_chains) *n_chains = (long long)n_traj * lag;
    if (n_chunks) *n_chunks = chunks;
    return DFF_OK;
}

extern "C" int dff_hmm_plan(const long long* lengths, int n_traj, int lag, long long* n_chains, long long* n_chunks) {
    return hmm_plan(lengths, n_traj, lag, n_chains, n_chunks, nullptr, "hmm_plan");
}

static int hmm_check_shape(long long n, int m, int K, const char* what) {
    if (n < 0) return fail(DFF_EINVAL, "%s: negative frame count", what);
    if (n > (1LL << 31)) return fail(DFF_EINVAL, "%s: more than 2^31 frames", what);
    if (m < 1 || m > DFF_HMM_MAXM) return fail(DFF_EINVAL, "%s: the number of hidden states must be 1..%d", what, DFF_HMM_MAXM);
    return micro_check_count(K, what, "symbols");
}

// the packed statistics of an E-step: loglik | xi (m, m) | gamma0 (m) | gamma_sym (m, K)
static long long hmm_nstats(int m, int K) { return 1 + (long long)m * m + m + (long long)m * K; }

// f(std::integral_constant<int, MP>()) for MP = hmm_pad(m): the one place that turns m hidden states into a template argument
template <class F>
static int hmm_with_pad(int m, F f) {
    switch (hmm_pad(m)) {
    case 2: return f(std::integral_constant<int, 2>());
    case 4: return f(std::integral_constant<int, 4>());
    default: return f(std::integral_constant<int, 8>());
    }
}

// a workspace cut into sections, each a multiple of 16 bytes.  Every hidden-Markov-model call starts its own with the
// trajectory table (HmmPlan) and the four flag words.
struct HmmSections {
    size_t total = 0, tab, flags;
    explicit HmmSections(int n_traj) {
        tab = take(2 * ((size_t)n_traj + 1) * sizeof(long long));
        flags = take(4 * sizeof(int));
    }
    size_t take(size_t bytes) {
        const size_t at = total;
        total += (bytes + 15) & ~(size_t)15;
        return at;
    }
};

struct HmmLayout : HmmSections {
    size_t a, p0, bt, prod, pexp, ain, bout, ll, post, part;
    HmmLayout(long long n, int n_traj, long long n_chains, long long n_chunks, int m, int K) : HmmSections(n_traj) {
        const size_t MP = (size_t)hmm_pad(m), d = sizeof(double);
        a = take(MP * MP * d);
        p0 = take(MP * d);
        bt = take((size_t)K * MP * d);
        prod = take((size_t)n_chunks * MP * MP * d);                // the chunk products, then the chunks' sums of xi
        pexp = take((size_t)n_chunks * MP * sizeof(int));
        ain = take((size_t)n_chunks * MP * d);
        bout = take((size_t)n_chunks * MP * d);
        ll = take((size_t)n_chains * d);
        post = take((size_t)n * m * d);
        part = take((size_t)((n + DFF_HMM_GROUP - 1) / DFF_HMM_GROUP) * K * m * d);
    }
};

// the bytes of a call whose workspace is a Layout, or -1 behind the refusal that the call itself would give
template <class Layout>
static long long hmm_workspace_bytes(const char* what, long long n, const long long* lengths, int n_traj, int lag, int m, int K) {
    if (hmm_check_shape(n, m, K, what)) return -1;
    long long n_chains, n_chunks;
    if (hmm_plan(lengths, n_traj, lag, &n_chains, &n_chunks, nullptr, what)) return -1;
    if (traj_check_lengths(lengths, n_traj, n, what)) return -1;
    return (long long)Layout(n, n_traj, n_chains, n_chunks, m, K).total;
}

extern "C" long long dff_hmm_workspace_bytes(long long n, const long long* lengths, int n_traj, int lag, int m, int K) {
    return hmm_workspace_bytes<HmmLayout>("hmm_workspace_bytes", n, lengths, n_traj, lag, m, K);
}

// What dff_hmm_estep, dff_hmm_fit_steps and dff_hmm_viterbi do before and after their own argument checks: check() is the
// refusals they share, in their order; workspace() follows the caller's own checks; upload(), behind ON_DEVICE, puts the
// trajectory table at the head of the workspace and names it in a plan.
struct HmmCall {
    const char* what;
    const long long* lengths = nullptr;
    int n_traj = 0, lag = 0;
    long long n_chains = 0, n_chunks = 0;
    std::vector<long long> tab;                                     // off[0 .. n_traj] | cpre[0 .. n_traj]; upload() fills off
    explicit HmmCall(const char* what) : what(what) {}

    // shape, null labels, plan, trajectory lengths
    int check(const int32_t* labels, long long n, const long long* lengths_, int n_traj_, int lag_, int m, int K) {
        lengths = lengths_, n_traj = n_traj_, lag = lag_;
        int rc = hmm_check_shape(n, m, K, what);
        if (rc) return rc;
        if (!labels && n > 0) return fail(DFF_EINVAL, "%s: null labels", what);
        tab.assign(2 * ((size_t)(n_traj > 0 ? n_traj : 0) + 1), 0);
        if ((rc = hmm_plan(lengths, n_traj, lag, &n_chains, &n_chunks, tab.data() + tab.size() / 2, what))) return rc;
        return traj_check_lengths(lengths, n_traj, n, what);
    }

    int workspace(const void* ws, size_t ws_bytes, const HmmSections& lay) const {
        const int rc = check_workspace(ws, ws_bytes, (long long)lay.total, what);
        if (rc) return rc;
        if ((uintptr_t)ws % sizeof(double)) return fail(DFF_EINVAL, "%s: the workspace must be 8-byte aligned", what);
        return DFF_OK;
    }

    int upload(hipStream_t stream, char* ws, const HmmSections& lay, HmmPlan* pl) {
        for (int r = 0; r < n_traj; ++r) tab[r + 1] = tab[r] + lengths[r];
        long long* dst = (long long*)(ws + lay.tab);
        pl->off = dst;
        pl->cpre = dst + tab.size() / 2;
        pl->n_traj = n_traj;
        pl->lag = lag;
        return upload_words(stream, tab.data(), (long long)tab.size(), dst);
    }
};

template <int MP>
static int hmm_launches(hipStream_t stream, const int32_t* labels, long long n, HmmPlan pl, long long n_chains, long long n_chunks,
                        int m, int K, const HmmLayout& lay, char* ws, double* stats, double* chain_ll, double* post) {
    const double* A = (const double*)(ws + lay.a);
    const double* p0 = (const double*)(ws + lay.p0);
    const double* Bt = (const double*)(ws + lay.bt);
    double* prod = (double*)(ws + lay.prod);
    int* pexp = (int*)(ws + lay.pexp);
    double* ain = (double*)(ws + lay.ain);
    double* bout = (double*)(ws + lay.bout);
    double* part = (double*)(ws + lay.part);
    int* flags = (int*)(ws + lay.flags);
    const long long n_groups = (n + DFF_HMM_GROUP - 1) / DFF_HMM_GROUP;
    const int stages = g_hmm_stages.load() ? g_hmm_stages.load() : 6;
    if (stages < 2) return DFF_OK;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(dff_hmm_products_kernel<MP>, dim3((unsigned)((n_chunks * MP + DFF_HMM_THREADS - 1) / DFF_HMM_THREADS)),
                           dim3(DFF_HMM_THREADS), 0, stream, labels, pl, n_chunks, m, K, A, Bt, prod, pexp);
        HIPCHK(hipGetLastError());
    }
    if (stages < 3) return DFF_OK;
    if (n_chains > 0) {
        hipLaunchKernelGGL(dff_hmm_carry_kernel<MP>, dim3((unsigned)((n_chains + 63) / 64), 2), dim3(64), 0, stream, labels, pl,
                           n_chains, m, K, p0, Bt, (const double*)prod, (const int*)pexp, ain, bout, chain_ll, flags);
        HIPCHK(hipGetLastError());
    }
    if (stages < 4) return DFF_OK;
    if (n_chunks > 0) {
        const int G = hmm_apply_groups(MP);
        const unsigned lds = (unsigned)((size_t)G * (DFF_HMM_CHUNK + 3) * MP * sizeof(double));
        if (lds > 48 * 1024)
            HIPCHK(hipFuncSetAttribute((const void*)&dff_hmm_apply_kernel<MP>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
        hipLaunchKernelGGL(dff_hmm_apply_kernel<MP>, dim3((unsigned)((n_chunks + G - 1) / G)), dim3(64), lds, stream, labels, pl,
                           n_chunks, m, K, A, p0, Bt, (const double*)ain, (const double*)bout, post, prod, flags);
        HIPCHK(hipGetLastError());
    }
    if (stages < 5) return DFF_OK;
    if (n_chunks > 0) {
        const unsigned elds = (unsigned)(((size_t)K * m + (size_t)DFF_HMM_GROUP * m) * sizeof(double) + DFF_HMM_GROUP * sizeof(int));
        if (elds > 48 * 1024)
            HIPCHK(hipFuncSetAttribute((const void*)&dff_hmm_emit_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)elds));
        hipLaunchKernelGGL(dff_hmm_emit_kernel, dim3((unsigned)n_groups), dim3(DFF_HMM_THREADS), elds, stream, labels, n, m, K,
                           (const double*)post, part);
        HIPCHK(hipGetLastError());
    }
    if (stages < 6) return DFF_OK;
    hipLaunchKernelGGL(dff_hmm_reduce_kernel<MP>, dim3((unsigned)hmm_nstats(m, K)), dim3(64), 0, stream, pl, n_chains, n_chunks, n_chunks > 0 ? n_groups : 0, m, K,
                       (const double*)chain_ll, (const double*)prod, (const double*)post, (const double*)part, stats);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

// One E-step on the stream: the parameters into the workspace, hmm_launches, then status and NaN.  dff_hmm_estep is one pass,
// dff_hmm_fit_steps one per iteration: the fit's E-step is this code, not a copy of it.  chain_loglik and post may be null: the
// launches then work in the workspace's sections, and finish gets them as given, so it only rewrites what the caller sees.
// With dff_debug_hmm_stages set the pass stops where hmm_launches stopped, before finish.
static int hmm_estep_pass(hipStream_t stream, const int32_t* labels, long long n, const HmmPlan& pl, const HmmCall& call,
                          const double* trans, const double* emit, const double* init, int m, int K, const HmmLayout& lay,
                          char* ws, double* stats, double* chain_loglik, double* post, int32_t* status) {
    hipLaunchKernelGGL(dff_hmm_prep_kernel, dim3(1), dim3(1024), 0, stream, trans, emit, init, m, K, hmm_pad(m),
                       (double*)(ws + lay.a), (double*)(ws + lay.p0), (double*)(ws + lay.bt), (int*)(ws + lay.flags));
    HIPCHK(hipGetLastError());
    double* ll = chain_loglik ? chain_loglik : (double*)(ws + lay.ll);
    double* pp = post ? post : (double*)(ws + lay.post);
    const int rc = hmm_with_pad(m, [&](auto mp) {
        return hmm_launches<decltype(mp)::value>(stream, labels, n, pl, call.n_chains, call.n_chunks, m, K, lay, ws, stats, ll, pp);
    });
    if (rc || g_hmm_stages.load()) return rc;
    const long long nstats = hmm_nstats(m, K);
    long long most = nstats > call.n_chains ? nstats : call.n_chains;
    if (post && n * m > most) most = n * m;
    const long long blocks = (most + DFF_HMM_THREADS - 1) / DFF_HMM_THREADS;
    hipLaunchKernelGGL(dff_hmm_finish_kernel, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(DFF_HMM_THREADS), 0, stream,
                       (const int*)(ws + lay.flags), nstats, stats, call.n_chains, chain_loglik, n * m, post, status);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

extern "C" int dff_hmm_estep(int device, const int32_t* labels, long long n, const long long* lengths, int n_traj, int lag,
                             const double* trans, const double* emit, const double* init, int m, int K, double* stats,
                             double* chain_loglik, double* post, int32_t* status, void* workspace, size_t workspace_bytes,
                             void* stream_) {
    HmmCall call("hmm_estep");
    int rc = call.check(labels, n, lengths, n_traj, lag, m, K);
    if (rc) return rc;
    if (!trans || !emit || !init || !stats || !status)
        return fail(DFF_EINVAL, "%s: null transition matrix / emissions / initial distribution / stats / status", call.what);
    const HmmLayout lay(n, n_traj, call.n_chains, call.n_chunks, m, K);
    if ((rc = call.workspace(workspace, workspace_bytes, lay))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    HmmPlan pl;
    if ((rc = call.upload(stream, ws, lay, &pl))) return rc;
    return hmm_estep_pass(stream, labels, n, pl, call, trans, emit, init, m, K, lay, ws, stats, chain_loglik, post, status);
}

// ---------------------------------------------------------------------------------------------
// Hidden Markov models: Baum-Welch on the device, n_steps iterations per call (dff_hmm_mstep.hip)
// ---------------------------------------------------------------------------------------------
static_assert(sizeof(dff_hmm_fit_state) == 32, "dff_hmm_fit_state is 32 bytes");

// the workspace of a fit: the sections of the E-step, then two more of the same kind, the E-step's packed statistics and its
// status word (one int in a section of 16 bytes)
struct HmmFitLayout : HmmLayout {
    size_t stats, status;
    HmmFitLayout(long long n, int n_traj, long long n_chains, long long n_chunks, int m, int K)
        : HmmLayout(n, n_traj, n_chains, n_chunks, m, K) {
        stats = take((size_t)hmm_nstats(m, K) * sizeof(double));
        status = take(sizeof(int));
    }
};

extern "C" long long dff_hmm_fit_workspace_bytes(long long n, const long long* lengths, int n_traj, int lag, int m, int K) {
    return hmm_workspace_bytes<HmmFitLayout>("hmm_fit_workspace_bytes", n, lengths, n_traj, lag, m, K);
}

extern "C" int dff_hmm_fit_steps(int device, const int32_t* labels, long long n, const long long* lengths, int n_traj, int lag,
                                 double* trans, double* emit, double* init, int m, int K, int reversible, int n_steps,
                                 double accuracy, double rev_tol, long long rev_max_sweeps, double* loglik, double* stationary,
                                 dff_hmm_fit_state* state, void* workspace, size_t workspace_bytes, void* stream_) {
    HmmCall call("hmm_fit_steps");
    const char* what = call.what;
    int rc = call.check(labels, n, lengths, n_traj, lag, m, K);
    if (rc) return rc;
    if (!trans || !emit || !init || !loglik || !state)
        return fail(DFF_EINVAL, "%s: null transition matrix / emissions / initial distribution / log-likelihoods / state", what);
    if (reversible != 0 && reversible != 1) return fail(DFF_EINVAL, "%s: reversible must be 0 or 1", what);
    if (n_steps < 1) return fail(DFF_EINVAL, "%s: n_steps must be >= 1", what);
    if (!(accuracy > 0.0)) return fail(DFF_EINVAL, "%s: accuracy must be > 0", what);
    if (!(rev_tol > 0.0)) return fail(DFF_EINVAL, "%s: rev_tol must be > 0", what);
    if (rev_max_sweeps < 1) return fail(DFF_EINVAL, "%s: rev_max_sweeps must be >= 1", what);
    if ((uintptr_t)state % sizeof(double)) return fail(DFF_EINVAL, "%s: the state must be 8-byte aligned", what);
    if (g_hmm_stages.load()) return fail(DFF_EINVAL, "%s: dff_debug_hmm_stages is set: the E-step would stop early", what);
    const HmmFitLayout lay(n, n_traj, call.n_chains, call.n_chunks, m, K);
    if ((rc = call.workspace(workspace, workspace_bytes, lay))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    HmmPlan pl;
    if ((rc = call.upload(stream, ws, lay, &pl))) return rc;     // once per call
    double* stats = (double*)(ws + lay.stats);
    int* status = (int*)(ws + lay.status);
    for (int s = 0; s < n_steps; ++s) {
        // the E-step of dff_hmm_estep, no output but its statistics and its status, both in the workspace
        if ((rc = hmm_estep_pass(stream, labels, n, pl, call, trans, emit, init, m, K, lay, ws, stats, nullptr, nullptr, status)))
            return rc;
        // control and M-step: one workgroup
        hipLaunchKernelGGL(dff_hmm_fit_mstep_kernel, dim3(1), dim3(DFF_HMM_FIT_THREADS), 0, stream, (const double*)stats,
                           (const int*)status, state, trans, emit, init, m, K, reversible, accuracy, rev_tol, rev_max_sweeps,
                           loglik + s, stationary);
        HIPCHK(hipGetLastError());
    }
    return DFF_OK;
}

// ---------------------------------------------------------------------------------------------
// Hidden Markov models: the most probable hidden path of every chain (dff_hmm_viterbi.hip)
// ---------------------------------------------------------------------------------------------
// how many of the call's launches run: 0 = all of them; 1 .. 6 = stop after the parameters, the chunk products, the forward
// carries, the apply pass, the backward carries, the backtrack (benchmarks: the share of every launch, by differences; the
// outputs are then unfinished)
static std::atomic<int> g_vit_stages{0};

extern "C" int dff_debug_hmm_viterbi_stages(int stages) {
    if (stages < 0 || stages > 6) return fail(DFF_EINVAL, "debug_hmm_viterbi_stages: 0 (all) or 1 .. 6 launches");
    g_vit_stages.store(stages);
    return DFF_OK;
}

struct VitLayout : HmmSections {
    size_t la, lp, lbt, prod, din, psi, origin, end, endstate, clp;
    VitLayout(long long n, int n_traj, long long n_chains, long long n_chunks, int m, int K) : HmmSections(n_traj) {
        const size_t MP = (size_t)hmm_pad(m), d = sizeof(double);
        la = take(MP * MP * d);
        lp = take(MP * d);
        lbt = take((size_t)K * MP * d);
        prod = take((size_t)n_chunks * MP * MP * d);
        din = take((size_t)n_chunks * MP * d);
        psi = take((size_t)n * sizeof(unsigned));                   // one word of back-pointers per frame, in chain order
        origin = take((size_t)n_chunks * sizeof(unsigned));
        end = take((size_t)n_chunks * sizeof(int));
        endstate = take((size_t)n_chains * sizeof(int));
        clp = take((size_t)n_chains * d);
    }
};

extern "C" long long dff_hmm_viterbi_workspace_bytes(long long n, const long long* lengths, int n_traj, int lag, int m, int K) {
    return hmm_workspace_bytes<VitLayout>("hmm_viterbi_workspace_bytes", n, lengths, n_traj, lag, m, K);
}

template <int MP>
static int vit_launches(hipStream_t stream, const int32_t* labels, HmmPlan pl, long long n_chains, long long n_chunks, int K,
                        const VitLayout& lay, char* ws, int32_t* path, int chain_order, double* chain_lp) {
    const double* la = (const double*)(ws + lay.la);
    const double* lp = (const double*)(ws + lay.lp);
    const double* lbt = (const double*)(ws + lay.lbt);
    double* prod = (double*)(ws + lay.prod);
    double* din = (double*)(ws + lay.din);
    unsigned* psi = (unsigned*)(ws + lay.psi);
    unsigned* origin = (unsigned*)(ws + lay.origin);
    int* end = (int*)(ws + lay.end);
    int* endstate = (int*)(ws + lay.endstate);
    int* flags = (int*)(ws + lay.flags);
    const int stages = g_vit_stages.load() ? g_vit_stages.load() : 7;
    const unsigned lane_blocks = (unsigned)((n_chunks * MP + DFF_VIT_THREADS - 1) / DFF_VIT_THREADS);
    if (stages < 2) return DFF_OK;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(dff_vit_products_kernel<MP>, dim3(lane_blocks), dim3(DFF_VIT_THREADS), 0, stream, labels, pl, n_chunks, K,
                           la, lbt, prod);
        HIPCHK(hipGetLastError());
    }
    if (stages < 3) return DFF_OK;
    if (n_chains > 0) {
        hipLaunchKernelGGL(dff_vit_forward_kernel<MP>, dim3((unsigned)((n_chains + 63) / 64)), dim3(64), 0, stream, labels, pl,
                           n_chains, K, lp, lbt, (const double*)prod, din, chain_lp);
        HIPCHK(hipGetLastError());
    }
    if (stages < 4) return DFF_OK;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(dff_vit_apply_kernel<MP>, dim3(lane_blocks), dim3(DFF_VIT_THREADS), 0, stream, labels, pl, n_chunks, K, la,
                           lbt, (const double*)din, psi, origin, endstate, chain_lp, flags);
        HIPCHK(hipGetLastError());
    }
    if (stages < 5) return DFF_OK;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(dff_vit_backward_kernel, dim3((unsigned)((n_chains + 63) / 64)), dim3(64), 0, stream, pl, n_chains,
                           (const unsigned*)origin, (const int*)endstate, end);
        HIPCHK(hipGetLastError());
    }
    if (stages < 6) return DFF_OK;
    if (n_chunks > 0) {
        hipLaunchKernelGGL(dff_vit_backtrack_kernel, dim3((unsigned)((n_chunks + DFF_VIT_THREADS - 1) / DFF_VIT_THREADS)),
                           dim3(DFF_VIT_THREADS), 0, stream, pl, n_chunks, (const unsigned*)psi, (const int*)end, chain_order, path);
        HIPCHK(hipGetLastError());
    }
    return DFF_OK;
}

extern "C" int dff_hmm_viterbi(int device, const int32_t* labels, long long n, const long long* lengths, int n_traj, int lag,
                               const double* logtrans, const double* logemit, const double* loginit, int m, int K, int32_t* path,
                               int chain_order, double* chain_logprob, int32_t* status, void* workspace, size_t workspace_bytes,
                               void* stream_) {
    HmmCall call("hmm_viterbi");
    const char* what = call.what;
    int rc = call.check(labels, n, lengths, n_traj, lag, m, K);
    if (rc) return rc;
    const long long n_chains = call.n_chains, n_chunks = call.n_chunks;
    if (!logtrans || !logemit || !loginit || !status || (!path && n > 0))
        return fail(DFF_EINVAL, "%s: null log transition matrix / log emissions / log initial distribution / path / status", what);
    if (chain_order != 0 && chain_order != 1) return fail(DFF_EINVAL, "%s: chain_order must be 0 (frame order) or 1 (chain order)", what);
    const VitLayout lay(n, n_traj, n_chains, n_chunks, m, K);
    if ((rc = call.workspace(workspace, workspace_bytes, lay))) return rc;
    ON_DEVICE(device);
    hipStream_t stream = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    HmmPlan pl;
    if ((rc = call.upload(stream, ws, lay, &pl))) return rc;
    HIPCHK(hipMemsetAsync(ws + lay.flags, 0, 4 * sizeof(int), stream));
    long long pblocks = (n + 1023) / 1024;
    pblocks = pblocks < 1 ? 1 : (pblocks > 1024 ? 1024 : pblocks);
    hipLaunchKernelGGL(dff_vit_prep_kernel, dim3((unsigned)pblocks), dim3(1024), 0, stream, labels, n, logtrans, logemit, loginit, m,
                       K, hmm_pad(m), (double*)(ws + lay.la), (double*)(ws + lay.lp), (double*)(ws + lay.lbt), (int*)(ws + lay.flags));
    HIPCHK(hipGetLastError());
    double* clp = chain_logprob ? chain_logprob : (double*)(ws + lay.clp);
    rc = hmm_with_pad(m, [&](auto mp) {
        return vit_launches<decltype(mp)::value>(stream, labels, pl, n_chains, n_chunks, K, lay, ws, path, chain_order, clp);
    });
    if (rc || g_vit_stages.load()) return rc;
    const long long most = n > n_chains ? n : n_chains;
    const long long blocks = (most + DFF_VIT_THREADS - 1) / DFF_VIT_THREADS;
    hipLaunchKernelGGL(dff_vit_finish_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks < 1024 ? blocks : 1024))), dim3(DFF_VIT_THREADS),
                       0, stream, (const int*)(ws + lay.flags), n, path, n_chains, chain_logprob, status);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}
