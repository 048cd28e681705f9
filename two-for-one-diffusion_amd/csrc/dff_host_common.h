// dff_host_common.h -- what the host translation units of libdff_amd.so (dff_host.hip: the model; dff_an_*.hip: the
// stateless sample-analysis entry points, which share dff_analysis_host.h on top of this; dff_loss.hip: the forward process and its loss) share: the error report behind dff_last_error, HIPCHK, the device guard.
// Host code only: no kernel file includes it.
#pragma once
#include "../../include/dff.h"
#include <hip/hip_runtime.h>

// records the message dff_last_error returns (thread-local, defined in dff_host.hip) and returns `code`; not part of the ABI
__attribute__((visibility("hidden"))) int fail(int code, const char* fmt, ...);
#define HIPCHK(x)                                                                              \
    do {                                                                                       \
        hipError_t e_ = (x);                                                                   \
        if (e_ != hipSuccess) return fail(DFF_EHIP, "%s failed: %s", #x, hipGetErrorString(e_)); \
    } while (0)

// The part of a model handle (private to dff_host.hip) that dff_loss.hip works from: the device, the sizes and the two
// forward-process schedule tables on the device (float32, `timesteps` entries each).  Defined in dff_host.hip.
struct DffLossView {
    int device, n_beads, timesteps;
    const float *sqrt_ac, *sqrt_1mac;   // sqrt_alphas_cumprod, sqrt_one_minus_alphas_cumprod
};
__attribute__((visibility("hidden"))) int dff_model_loss_view(const dff_model* m, DffLossView* v);

// Every ABI entry runs on the model's device and leaves the caller's current device as it found it (a process that
// drives several GPUs keeps torch's notion of the current device).
struct DeviceGuard {
    int prev = -1;
    bool ok = true;
    explicit DeviceGuard(int dev) {
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) { ok = false; return; }
        if (cur != dev) {
            if (hipSetDevice(dev) != hipSuccess) { ok = false; return; }
            prev = cur;
        }
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard&) = delete;
    DeviceGuard& operator=(const DeviceGuard&) = delete;
};
#define ON_DEVICE(dev)                                                         \
    DeviceGuard dev_guard_(dev);                                               \
    if (!dev_guard_.ok) return fail(DFF_EHIP, "cannot select device %d", (int)(dev))
