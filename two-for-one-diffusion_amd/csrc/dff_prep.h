// dff_prep.h -- weight preparation (dff_prep.hip): everything between "a config and a flat weight array" and "host images
// ready to upload".  Pure CPU work, no HIP runtime call; dff_host.hip uploads what it returns.
#pragma once
#include "../../include/dff.h"
#include <cstdint>
#include <functional>
#include <string>
#include <vector>
#pragma GCC visibility push(hidden)   // internal to the library, like fail() of dff_host_common.h
namespace dff_prep {

// one weight-GEMM operand: element (k, n) of a (K x Nout) matrix, float64 where it is a fold product
struct Operand {
    int K, Nout;
    std::function<double(int, int)> w;
};
// fp32 image for the v_mfma_f32_16x16x4_f32 B operand (layout: dff_internal.h); also packs dff_debug_gemm's matrix
std::vector<float> pack_b(const Operand& op, int xper = 0);

// the images of one layer, named as the DffLayerDev members (dff_internal.h) they are uploaded to
// (uint32_t: two fp16 pieces per weight; empty where the model does not run that engine -- `split`: *_s, `small_split`: *_w / *_t)
#define DFF_LAYER_IMAGES(X) X(float, ln1_g) X(float, ln1_b) X(float, bo) X(float, g1) X(float, ln2_g) X(float, ln2_b) X(float, W1_p) X(float, b1) \
    X(float, W2_p) X(float, b2) X(float, g2) X(float, W2T_p) X(float, W1T_p) X(float, Wqkvx_p) X(float, bqkvx) X(float, Wox_p) X(float, WoxT_p) \
    X(float, WqkvxT_p) X(uint32_t, Wqkvx_s) X(uint32_t, W1_s) X(uint32_t, W2T_s) X(uint32_t, WoxT_s) X(uint32_t, W2_s) X(uint32_t, W1T_s) \
    X(uint32_t, Wox_s) X(uint32_t, WqkvxT_s) X(uint32_t, Wqkvx_w) X(uint32_t, W1_w) X(uint32_t, W2T_w) X(uint32_t, WoxT_w) X(uint32_t, Wox_t) \
    X(uint32_t, W2_t) X(uint32_t, W1T_t) X(uint32_t, WqkvxT_t)
struct PrepLayer {
#define X(T, n) std::vector<T> n;
    DFF_LAYER_IMAGES(X)
#undef X
};

struct DffPrep {
    bool split;         // fp16 images exist, SPW variants preferred
    bool small_split;   // ... and the <= 16-row kernel has an SPW variant for this model
    bool fold_kv;       // H == 64: k = v = LayerNorm output (W_k folded into W_q, W_v into W_o)
    std::string note;   // the range guard's message when it takes a model off the fp16 engine (for stderr), else empty
    std::vector<float> WnT, bn, wdec;       // node embedding (transposed) and decoder head
    float bdec, bdec3[3];
    std::vector<PrepLayer> layer;
    std::vector<std::vector<float>> sched;  // 12 schedule tables, host fp32
};
// want_split / want_fold: what the caller's policy allows (DFF_SPLIT_BF16, DFF_FOLD_KV); small_spw: the model fits the <= 16-row
// kernel's SPW variant and this build has one for cfg.hidden.  cfg and the weight count have been checked.
DffPrep dff_prepare(const dff_config& cfg, const float* w, bool want_split, bool want_fold, bool small_spw);
}   // namespace dff_prep
#pragma GCC visibility pop
