// dff_upload.h -- host tables (segment starts, problem descriptors, bin counts) travel into a workspace as kernel ARGUMENTS,
// DFF_MSMB_UPLOAD 64-bit words per launch: ordered on the stream, no host-to-device copy that could wait for it.  The kernel,
// dff_msmb_upload_kernel, is compiled once (dff_msm_batch.hip); every analysis unit uploads through upload_words.
#pragma once
#include <hip/hip_runtime.h>

#define DFF_MSMB_UPLOAD 448          // 64-bit words per upload launch: 3.5 KB of kernel arguments

struct MsmbWords {
    long long v[DFF_MSMB_UPLOAD];
};

// `cnt` 64-bit words of a host table into the workspace, as kernel arguments: nothing the stream could make the host wait for (defined in dff_an_markov.hip)
__attribute__((visibility("hidden"))) int upload_words(hipStream_t stream, const long long* src, long long cnt, long long* dst);
