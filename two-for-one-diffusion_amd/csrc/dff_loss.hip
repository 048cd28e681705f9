// dff_loss.hip -- the forward process and its loss: q_sample, p_losses (models/ddpm.py:265-315) around the score op.
// Two small kernels, one wave per sample (lane = bead, N <= 64: the bead means are one butterfly over the wave, the same
// order every time), and the host code of dff_q_sample / dff_denoise_loss (include/dff.h).  The score itself goes through
// dff_score -- the one launch path of dff_host.hip -- so every configuration that scores can be scored against a
// validation set, and no kernel variant is added.
#include "../../include/dff.h"
#include "dff_device.h"
#include "dff_host_common.h"

#include <cmath>

#define DFF_FWD_STEP 0xFFFFFFFE00000000ull   // high word of the Philox step of forward-process draws (dff.h); low word = draw
#define DFF_LOSS_WAVES 4                      // samples per 256-thread workgroup
#define DFF_LOSS_CHUNK 16384                  // samples per pass: bounds the workspace (x_t, tnorm, model output)
#define DFF_LOSS_PARTS 256                    // at most this many first-stage partial sums

template <class T> DEVI T wave_sum(T v) {   // butterfly: every lane ends with the same sum, added in the same order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// z[c] of bead `lane` of sample b: supplied, or drawn (item, step, bead) as the samplers draw; 0 on the lanes past N
DEVI void load_noise(const float* __restrict__ noise, size_t b, int N, int lane, uint64_t seed, uint64_t item, uint64_t step,
                     float (&z)[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (lane >= N) z[c] = 0.f;
        else if (noise) z[c] = noise[(b * N + lane) * 3 + c];
        else z[c] = philox_normal(seed, item, step, (uint32_t)lane, c);
    }
}

// xt[b] = center_zero(sqrt_ac[t_b] x0[b] + sqrt_1mac[t_b] center_zero(z[b])), tnorm[b] = t_b / T; fp32, the products and the
// sum rounded separately as torch rounds them.  A level outside 0 .. T - 1 gives NaN outputs for that sample.
__global__ __launch_bounds__(64 * DFF_LOSS_WAVES) void dff_q_sample_kernel(
    const float* __restrict__ x0, const int32_t* __restrict__ t, const float* __restrict__ noise, uint64_t seed, uint64_t item0,
    uint64_t step, const float* __restrict__ sqrt_ac, const float* __restrict__ sqrt_1mac, int N, int T, int B,
    float* __restrict__ xt, float* __restrict__ tnorm) {
    const int lane = threadIdx.x & 63;
    const size_t b = (size_t)blockIdx.x * DFF_LOSS_WAVES + (threadIdx.x >> 6);
    if (b >= (size_t)B) return;   // (wave-uniform; the kernel has no workgroup barrier)
    const int tb = t[b];
    const bool ok = tb >= 0 && tb < T;
    const float a = ok ? sqrt_ac[tb] : 0.f, s = ok ? sqrt_1mac[tb] : 0.f;
    const float nf = (float)N;
    float z[3], y[3];
    load_noise(noise, b, N, lane, seed, item0 + b, step, z);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float zc = z[c] - wave_sum(z[c]) / nf;
        const float x = lane < N ? x0[(b * N + lane) * 3 + c] : 0.f;
        y[c] = lane < N ? __fadd_rn(__fmul_rn(a, x), __fmul_rn(s, zc)) : 0.f;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float yc = y[c] - wave_sum(y[c]) / nf;
        if (lane < N) xt[(b * N + lane) * 3 + c] = ok ? yc : __builtin_nanf("");
    }
    if (lane == 0 && tnorm) tnorm[b] = ok ? (float)tb / (float)T : __builtin_nanf("");
}

// loss[b] = mean over the 3 N entries of |d| (loss_type 1) or d^2 (2), d = center_zero(out[b]) - center_zero(z[b]); the
// means, the differences and the sum in fp64, one rounding to fp32 at the end.  NaN for a level outside 0 .. T - 1.
__global__ __launch_bounds__(64 * DFF_LOSS_WAVES) void dff_loss_kernel(
    const float* __restrict__ out, const int32_t* __restrict__ t, const float* __restrict__ noise, uint64_t seed, uint64_t item0,
    uint64_t step, int N, int T, int B, int loss_type, float* __restrict__ loss) {
    const int lane = threadIdx.x & 63;
    const size_t b = (size_t)blockIdx.x * DFF_LOSS_WAVES + (threadIdx.x >> 6);
    if (b >= (size_t)B) return;
    const int tb = t[b];
    float z[3];
    load_noise(noise, b, N, lane, seed, item0 + b, step, z);
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double o = lane < N ? (double)out[(b * N + lane) * 3 + c] : 0.0;
        const double d = (o - wave_sum(o) / N) - ((double)z[c] - wave_sum((double)z[c]) / N);
        if (lane < N) acc += loss_type == 1 ? fabs(d) : d * d;
    }
    acc = wave_sum(acc) / (3.0 * N);
    if (lane == 0) loss[b] = (tb >= 0 && tb < T) ? (float)acc : __builtin_nanf("");
}

// total: a two-stage sum in a fixed order.  Stage one: workgroup p adds loss[p per .. (p + 1) per) (strided over its threads,
// then a tree in LDS); stage two: one workgroup adds the <= 256 partials by the same tree and updates total[0], total[1].
DEVI double block_sum_256(double v, double* sh) {
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) sh[threadIdx.x] += sh[threadIdx.x + s];
        __syncthreads();
    }
    return sh[0];
}
__global__ __launch_bounds__(256) void dff_loss_partial_kernel(const float* __restrict__ loss, int B, long long per,
                                                               double* __restrict__ partial) {
    __shared__ double sh[256];
    const long long lo = blockIdx.x * per, hi = lo + per < B ? lo + per : B;
    double acc = 0.0;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) acc += (double)loss[i];
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) partial[blockIdx.x] = acc;
}
__global__ __launch_bounds__(256) void dff_loss_total_kernel(const double* __restrict__ partial, int parts, int B,
                                                             double* __restrict__ total) {
    __shared__ double sh[256];
    const double s = block_sum_256((int)threadIdx.x < parts ? partial[threadIdx.x] : 0.0, sh);
    if (threadIdx.x == 0) { total[0] += s; total[1] += (double)B; }
}

// ------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------
static bool items_ok(uint64_t offset, int count) {   // offset + count <= 2^40 (the counter layout, dff.h)
    const uint64_t lim = 1ull << 40;
    return offset <= lim && (uint64_t)count <= lim - offset;
}

static int q_sample_launch(const DffLossView& v, const float* x0, const int32_t* t, int n, const float* noise, uint64_t seed,
                           uint64_t item0, uint64_t step, float* xt, float* tnorm, hipStream_t stream) {
    hipLaunchKernelGGL(dff_q_sample_kernel, dim3((n + DFF_LOSS_WAVES - 1) / DFF_LOSS_WAVES), dim3(64 * DFF_LOSS_WAVES), 0, stream,
                       x0, t, noise, seed, item0, step, v.sqrt_ac, v.sqrt_1mac, v.n_beads, v.timesteps, n, xt, tnorm);
    HIPCHK(hipGetLastError());
    return DFF_OK;
}

static int forward_args(const dff_model* m, const float* x0, const int32_t* t, int batch, const float* noise,
                        uint64_t sample_offset, DffLossView* v) {
    if (!m || !x0 || !t) return fail(DFF_EINVAL, "null argument");
    if (batch < 0) return fail(DFF_EINVAL, "negative batch");
    if (!noise && !items_ok(sample_offset, batch))
        return fail(DFF_EINVAL, "sample_offset + batch = %llu + %d exceeds 2^40: the in-kernel noise is keyed by 40 bits of the sample index",
                    (unsigned long long)sample_offset, batch);
    return dff_model_loss_view(m, v);
}

extern "C" int dff_q_sample(dff_model* m, const float* x0, const int32_t* t, int batch, const float* noise, uint64_t seed,
                            uint64_t sample_offset, uint32_t draw, float* xt, float* tnorm, void* stream) {
    DffLossView v;
    if (int rc = forward_args(m, x0, t, batch, noise, sample_offset, &v)) return rc;
    if (!xt) return fail(DFF_EINVAL, "null argument");
    if (batch == 0) return DFF_OK;
    ON_DEVICE(v.device);
    return q_sample_launch(v, x0, t, batch, noise, seed, sample_offset, DFF_FWD_STEP | draw, xt, tnorm, (hipStream_t)stream);
}

static long long workspace_bytes(int n_beads, int batch) {
    const long long c = batch < DFF_LOSS_CHUNK ? batch : DFF_LOSS_CHUNK;
    return DFF_LOSS_PARTS * (long long)sizeof(double) + c * (6 * n_beads + 1) * (long long)sizeof(float);
}

extern "C" long long dff_denoise_workspace_bytes(const dff_model* m, int batch) {
    DffLossView v;
    if (batch < 0 || dff_model_loss_view(m, &v)) { fail(DFF_EINVAL, "bad workspace request"); return -1; }
    return workspace_bytes(v.n_beads, batch);
}

extern "C" int dff_denoise_loss(dff_model* m, const float* x0, const int32_t* t, int batch, const float* noise, uint64_t seed,
                                uint64_t sample_offset, uint32_t draw, int loss_type, float* loss, double* total, float* xt_out,
                                float* model_out, void* workspace, size_t workspace_bytes_, void* stream_) {
    DffLossView v;
    if (int rc = forward_args(m, x0, t, batch, noise, sample_offset, &v)) return rc;
    if (!loss) return fail(DFF_EINVAL, "null argument");
    if (loss_type != 1 && loss_type != 2) return fail(DFF_EINVAL, "invalid loss type %d (1 = l1, 2 = l2)", loss_type);
    if (batch == 0) return DFF_OK;
    if (!workspace || ((uintptr_t)workspace & 7) || (long long)workspace_bytes_ < workspace_bytes(v.n_beads, batch))
        return fail(DFF_EINVAL, "workspace of %zu bytes: need %lld, 8-byte aligned (dff_denoise_workspace_bytes)", workspace_bytes_,
                    workspace_bytes(v.n_beads, batch));
    hipStream_t stream = (hipStream_t)stream_;
    ON_DEVICE(v.device);
    const int N = v.n_beads, cmax = batch < DFF_LOSS_CHUNK ? batch : DFF_LOSS_CHUNK;
    const size_t row = (size_t)N * 3;
    double* partial = (double*)workspace;
    float* xt = (float*)(partial + DFF_LOSS_PARTS);
    float* out = xt + cmax * row;
    float* tn = out + cmax * row;
    const uint64_t step = DFF_FWD_STEP | draw;
    // a batch beyond the chunk runs as consecutive passes over one workspace: samples are independent, and the stream orders
    // the passes; inside a pass the score cuts the batch at the model's workgroup limit as it always does
    for (int b0 = 0; b0 < batch; b0 += cmax) {
        const int n = batch - b0 < cmax ? batch - b0 : cmax;
        const float* nz = noise ? noise + b0 * row : nullptr;
        if (int rc = q_sample_launch(v, x0 + b0 * row, t + b0, n, nz, seed, sample_offset + b0, step, xt, tn, stream)) return rc;
        if (int rc = dff_score(m, xt, tn, n, out, nullptr, stream_)) return rc;
        hipLaunchKernelGGL(dff_loss_kernel, dim3((n + DFF_LOSS_WAVES - 1) / DFF_LOSS_WAVES), dim3(64 * DFF_LOSS_WAVES), 0, stream,
                           (const float*)out, t + b0, nz, seed, sample_offset + b0, step, N, v.timesteps, n, loss_type, loss + b0);
        HIPCHK(hipGetLastError());
        if (xt_out) HIPCHK(hipMemcpyAsync(xt_out + b0 * row, xt, n * row * sizeof(float), hipMemcpyDeviceToDevice, stream));
        if (model_out) HIPCHK(hipMemcpyAsync(model_out + b0 * row, out, n * row * sizeof(float), hipMemcpyDeviceToDevice, stream));
    }
    if (total) {
        long long per = ((long long)batch + DFF_LOSS_PARTS - 1) / DFF_LOSS_PARTS;
        if (per < 256) per = 256;
        const int parts = (int)((batch + per - 1) / per);
        hipLaunchKernelGGL(dff_loss_partial_kernel, dim3(parts), dim3(256), 0, stream, (const float*)loss, batch, per, partial);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(dff_loss_total_kernel, dim3(1), dim3(256), 0, stream, (const double*)partial, parts, batch, total);
        HIPCHK(hipGetLastError());
    }
    return DFF_OK;
}
