// dff_prep.hip -- weight preparation for libdff_amd.so: the layout of the flat weight array, the float64 folds, the fp16 engine's
// range guard, the MFMA operand images (fp32 and two-piece fp16), the schedule tables.  No HIP runtime call: dff_host.hip uploads.
#include "dff_prep.h"
#include "dff_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>

namespace dff_prep {
// ---- the flat weight array (the reference's registration order, graph_transformer.py) ----
namespace {
struct Cursor {   // w == nullptr: counts only
    const float* w;
    size_t off = 0;
    const float* take(size_t n) { const float* r = w ? w + off : nullptr; off += n; return r; }
};
struct EmbedWeights {
    size_t NI;    // node inputs: one-hot (N) | x (3, with abs coords) | t
    size_t nfe;   // edge inputs: x_j - x_i (3) | |x_j - x_i|^2 ; neither -> one zero feature
    size_t dec;   // node_decoder: Linear(H, 1) or Linear(H, 3)
    const float *Wn, *bn, *We, *be, *wd, *bd;
};
struct LayerWeights {
    const float *Wq, *bq, *Wkv, *bkv, *Wek, *bek, *Wo, *bo, *ln1g, *ln1b, *g1, *W1, *b1, *W2, *b2, *ln2g, *ln2b, *g2;
};
// H == head dimension: the k / v fold's products (float64).  logits: q.k_j = (W_k,h^T q_i).n_j + [constant in j], so with
// q'_ih = W_k,h^T (W_q,h n_i + b_q,h) the keys are the LayerNorm rows n_j themselves; values: W_o,h sum_j a_ij (W_v,h n_j + b_v,h)
// = (W_o,h W_v,h) sum_j a_ij n_j + W_o,h b_v,h.
struct KvFold {
    std::vector<double> Mq, cq, Wof;   // W_k,h^T W_q,h (I x H), W_k,h^T b_q,h (I), W_o,h W_v,h (H x I)
};
}   // namespace
static EmbedWeights cut_embed(Cursor& c, const dff_config& cfg) {
    const size_t H = cfg.hidden;
    EmbedWeights e;
    e.NI = (size_t)cfg.n_beads + 1 + (cfg.use_abs_coords ? 3 : 0);                          // graph_transformer.py:53
    e.nfe = (cfg.use_intrinsic_coords ? 3 : 0) + (cfg.use_distances ? 1 : 0);               // :54-58
    if (e.nfe == 0) e.nfe = 1;
    e.dec = cfg.conservative ? 1 : 3;
    e.Wn = c.take(H * e.NI); e.bn = c.take(H);
    e.We = c.take(H * e.nfe); e.be = c.take(H);
    e.wd = c.take(e.dec * H); e.bd = c.take(e.dec);
    return e;
}
static LayerWeights cut_layer(Cursor& c, size_t H) {
    const size_t I = DFF_INNER, F = 4 * H;
    LayerWeights l;
    l.Wq = c.take(I * H); l.bq = c.take(I);
    l.Wkv = c.take(2 * I * H); l.bkv = c.take(2 * I);
    l.Wek = c.take(I * H); l.bek = c.take(I);
    l.Wo = c.take(H * I); l.bo = c.take(H);
    l.ln1g = c.take(H); l.ln1b = c.take(H); l.g1 = c.take(3 * H);
    l.W1 = c.take(F * H); l.b1 = c.take(F);
    l.W2 = c.take(H * F); l.b2 = c.take(H);
    l.ln2g = c.take(H); l.ln2b = c.take(H); l.g2 = c.take(3 * H);
    return l;
}
}   // namespace dff_prep
extern "C" size_t dff_weight_count(const dff_config* c) {
    using namespace dff_prep;
    if (!c) return 0;
    Cursor cur{nullptr};
    cut_embed(cur, *c);
    const size_t n = cur.off;
    cut_layer(cur, c->hidden);
    return n + (cur.off - n) * c->n_layers;
}

namespace dff_prep {
// ---- packing for the v_mfma_f32_16x16x4_f32 B operand (layout: dff_internal.h) ----
// xper > 0: k-blocks with kb % xper == 4 are head EXTENSION blocks, of which only rows 0..3 are ever non-zero
// (u | s, xrel | D, du | ds): they are packed with row (lane >> 4) in k-step 0 and zeros in k-steps 1..3, and the
// kernels issue one MFMA for them instead of four (A operand: column lane >> 4 of the block).
std::vector<float> pack_b(const Operand& op, int xper) {
    const int K = op.K, Nout = op.Nout, KB = (K + 15) / 16, NT = (Nout + 15) / 16;
    std::vector<float> out((size_t)KB * NT * 256, 0.f);
    for (int nt = 0; nt < NT; ++nt)
        for (int kb = 0; kb < KB; ++kb) {
            const bool ext = xper > 0 && kb % xper == 4;
            for (int lane = 0; lane < 64; ++lane)
                for (int s = 0; s < (ext ? 1 : 4); ++s) {
                    const int k = 16 * kb + (ext ? lane >> 4 : 4 * (lane >> 4) + s), n = 16 * nt + (lane & 15);
                    if (k < K && n < Nout) out[(((size_t)nt * KB + kb) * 64 + lane) * 4 + s] = (float)op.w(k, n);
                }
        }
    return out;
}

// fp32 -> fp16 (binary16), round to nearest even, subnormals kept: what v_cvt_pk_f16_f32 does on the device (dff_device.h split2h)
static uint16_t f32_to_f16_rn(float f) {
    uint32_t u; memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u, a = u & 0x7fffffffu;
    if (a >= 0x7f800000u) return (uint16_t)(sign | 0x7c00u | ((a > 0x7f800000u) ? 0x200u : 0u));   // inf / nan
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);             // >= 65520 rounds to infinity (the range guard keeps models away)
    const int e = (int)(a >> 23) - 127;
    if (e < -25) return (uint16_t)sign;                                   // < 2^-25: zero
    uint32_t r, rem, half;
    if (e >= -14) { r = (uint32_t)(e + 15) << 10 | ((a >> 13) & 0x3ffu); rem = a & 0x1fffu; half = 0x1000u; }
    else {                                                                // subnormal: value = mant 2^(e - 23) = r 2^-24
        const uint32_t mant = (a & 0x7fffffu) | 0x800000u; const int sh = -e - 1;   // 14 .. 24
        r = mant >> sh; rem = mant & ((1u << sh) - 1u); half = 1u << (sh - 1);
    }
    if (rem > half || (rem == half && (r & 1u))) ++r;                     // (a carry out of the mantissa lands in the exponent: right)
    return (uint16_t)(sign | r);
}
static float f16_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, mnt = h & 0x3ffu;
    float f;
    if (e == 0) { f = (float)mnt * 5.9604644775390625e-08f; uint32_t u; memcpy(&u, &f, 4); u |= sign; memcpy(&f, &u, 4); return f; }
    const uint32_t u = sign | ((e == 31 ? 255u : e + 112u) << 23) | (mnt << 13);
    memcpy(&f, &u, 4);
    return f;
}
// The split engine's images are sequences of UNITS, each one 16-column output tile nt x 32 k-rows starting at c0 = 32 kb, ordered
// [tile][k-block] or, `tall`, [k-block][tile], and stored [piece h | l'][lane][8 fp16], two per dword (even j in the low half);
// h = RN_f16(w), l' = RN_f16((w - h) 2048): w = h + l' / 2048 to 2^-22 relative (3e-11 absolute).
// krow(lane, j): the row, inside its unit's 32, that element j of lane (n = lane & 15, kg = lane >> 4) holds
static std::vector<uint32_t> pack_f16(const Operand& op, bool tall, int (*krow)(int, int)) {
    const int KB = op.K / 32, NT = (op.Nout + 15) / 16;
    std::vector<uint32_t> out((size_t)NT * KB * 2 * 64 * 4, 0u);
    for (int u = 0; u < NT * KB; ++u)
        for (int lane = 0; lane < 64; ++lane)
            for (int j = 0; j < 8; ++j) {
                const int k = 32 * (tall ? u / NT : u % KB) + krow(lane, j), n = 16 * (tall ? u % NT : u / KB) + (lane & 15);
                const float v = n < op.Nout ? (float)op.w(k, n) : 0.f;
                const uint16_t h = f32_to_f16_rn(v);
                const uint16_t l = f32_to_f16_rn((v - f16_to_f32(h)) * 2048.0f);
                out[(((size_t)u * 2 + 0) * 64 + lane) * 4 + (j >> 1)] |= (uint32_t)h << (16 * (j & 1));
                out[(((size_t)u * 2 + 1) * 64 + lane) * 4 + (j >> 1)] |= (uint32_t)l << (16 * (j & 1));
            }
    return out;
}
// B operand of v_mfma_f32_16x16x32_f16 for the split GEMMs of the <= 64-row kernel (dff_kernels.hip gemm_wide_split_st and
// friends): units [tile][k-block], lane holds W[32 kb + 8 (lane >> 4) + j][16 nt + (lane & 15)], j = 0..7
static std::vector<uint32_t> pack_b_split_f16(const Operand& op) {
    return pack_f16(op, false, [](int lane, int j) { return 8 * (lane >> 4) + j; });
}
// Split images for the <= 16-row kernel's SPW variants (dff_small.hip): element j of lane is W(c0 + 16 (j >> 2) + 4 kg + (j & 3),
// 16 nt + n): the k order in which that kernel's A fragments hold a 32-column block (two ds_read_b128, at columns 4 kg and
// 16 + 4 kg).
static std::vector<uint32_t> pack_units_f16(const Operand& op, bool tall) {
    return pack_f16(op, tall, [](int lane, int j) { return 16 * (j >> 2) + 4 * (lane >> 4) + (j & 3); });
}

// cosine schedule + derived tables, float64 -> float32  (utils.py:52-62, models/ddpm.py:52-99)
static void build_schedule(int T, std::vector<std::vector<float>>& out) {
    const double s = 0.008, pi = 3.14159265358979323846;
    std::vector<double> ac0(T + 1), betas(T), alphas(T), ac(T), acp(T);
    for (int i = 0; i <= T; ++i) {
        const double x = (double)i;  // torch.linspace(0, T, T+1) is exact for integer steps
        const double cv = std::cos(((x / T) + s) / (1 + s) * pi * 0.5);
        ac0[i] = cv * cv;
    }
    for (int i = T; i >= 0; --i) ac0[i] = ac0[i] / ac0[0];
    for (int i = 0; i < T; ++i) {
        double b = 1 - (ac0[i + 1] / ac0[i]);
        betas[i] = b < 0 ? 0 : (b > 0.999 ? 0.999 : b);
        alphas[i] = 1.0 - betas[i];
    }
    double cp = 1.0;
    for (int i = 0; i < T; ++i) { cp *= alphas[i]; ac[i] = cp; }
    for (int i = 0; i < T; ++i) acp[i] = i == 0 ? 1.0 : ac[i - 1];
    out.assign(12, std::vector<float>(T));
    for (int i = 0; i < T; ++i) {
        const double pv = betas[i] * (1.0 - acp[i]) / (1.0 - ac[i]);
        out[0][i] = (float)betas[i];
        out[1][i] = (float)ac[i];
        out[2][i] = (float)acp[i];
        out[3][i] = (float)std::sqrt(ac[i]);
        out[4][i] = (float)std::sqrt(1.0 - ac[i]);
        out[5][i] = (float)std::log(1.0 - ac[i]);
        out[6][i] = (float)std::sqrt(1.0 / ac[i]);
        out[7][i] = (float)std::sqrt(1.0 / ac[i] - 1);
        out[8][i] = (float)pv;
        out[9][i] = (float)std::log(pv < 1e-20 ? 1e-20 : pv);
        out[10][i] = (float)(betas[i] * std::sqrt(acp[i]) / (1.0 - ac[i]));
        out[11][i] = (float)((1.0 - acp[i]) * std::sqrt(alphas[i]) / (1.0 - ac[i]));
    }
}

static KvFold kv_fold(const LayerWeights& w) {
    const int H = DFF_DH, I = DFF_INNER;
    KvFold f;
    f.Mq.assign((size_t)I * H, 0.0); f.cq.assign(I, 0.0); f.Wof.assign((size_t)H * I, 0.0);
    for (int h = 0; h < DFF_HEADS; ++h)
        for (int e = 0; e < DFF_DH; ++e) {
            for (int c = 0; c < H; ++c) {
                double sq = 0, so = 0;
                for (int dd = 0; dd < DFF_DH; ++dd) {
                    sq += (double)w.Wkv[(size_t)(h * 64 + dd) * H + e] * w.Wq[(size_t)(h * 64 + dd) * H + c];
                    so += (double)w.Wo[(size_t)c * I + h * 64 + dd] * w.Wkv[(size_t)(I + h * 64 + dd) * H + e];
                }
                f.Mq[(size_t)(h * 64 + e) * H + c] = sq;
                f.Wof[(size_t)c * I + h * 64 + e] = so;
            }
            double sc = 0;
            for (int dd = 0; dd < DFF_DH; ++dd) sc += (double)w.Wkv[(size_t)(h * 64 + dd) * H + e] * w.bq[h * 64 + dd];
            f.cq[h * 64 + e] = sc;
        }
    return f;
}

// ---- the fp16 engine's range guard ----
// The fp16 pieces of the FORWARD GEMM inputs are taken of the activations as they are (dff_device.h split8h): LayerNorm
// outputs, attention outputs (averages of v), GELU(hidden).  Their worst-case magnitudes follow from the weights alone;
// a model that could take them past fp16's range (|x| < 1.6e4 keeps x and its 2^11-scaled low piece finite) runs the
// fp32 engine instead.  (The backward's inputs are scaled on the device.)  Trained models are orders of magnitude away.
// Returns the message for stderr when the model has to leave the engine, else an empty string.  kv: the fold products per layer
// (empty unless H == 64 && L <= 3).
static std::string range_guard(const std::vector<LayerWeights>& layers, int H, const std::vector<KvFold>& kv) {
    const int I = DFF_INNER, F = 4 * H;
    auto amax = [](const float* a, size_t n) { double mx = 0; for (size_t i = 0; i < n; ++i) mx = std::max(mx, (double)fabsf(a[i])); return mx; };
    auto rowl1 = [](const float* a, int rows, int cols) {   // largest L1 norm of a row of a (rows x cols) matrix
        double mx = 0;
        for (int r = 0; r < rows; ++r) { double t = 0; for (int c = 0; c < cols; ++c) t += fabs((double)a[(size_t)r * cols + c]); mx = std::max(mx, t); }
        return mx;
    };
    double worst = 0;
    // ... and the low end: a piece resolves 2^-25 / 2^11 = 2^-36 absolutely (fp16's subnormal spacing below 2^-14), so an
    // operand whose largest entry is below 2^-12 no longer gets the format's 2^-22 relative accuracy.  `least` is the
    // smallest of the GEMM weights' max|w| (exact zeros are exact pieces: skipped) and of the LayerNorm rows' bounds.
    double least = INFINITY;
    auto low = [&](double v) { if (v > 0) least = std::min(least, v); };
    for (size_t l = 0; l < layers.size(); ++l) {
        const LayerWeights& w = layers[l];
        const double m1 = sqrt((double)H) * amax(w.ln1g, H) + amax(w.ln1b, H);
        const double m2 = sqrt((double)H) * amax(w.ln2g, H) + amax(w.ln2b, H);
        const double vb = rowl1(w.Wkv + (size_t)I * H, I, H) * m1 + amax(w.bkv + I, I);   // |v| (and their attention averages)
        const double hb = rowl1(w.W1, F, H) * m2 + amax(w.b1, F);                          // |h_pre| >= |GELU(h_pre)|
        worst = std::max(std::max(worst, m1), std::max(std::max(m2, vb), hb));
        // the weights themselves become fp16 pieces too (f32_to_f16_rn maps |w| >= 65520 to infinity)
        const double aq = amax(w.Wq, (size_t)I * H), ak = amax(w.Wkv, (size_t)I * H), av = amax(w.Wkv + (size_t)I * H, (size_t)I * H),
                     ae = amax(w.Wek, (size_t)I * H), ao = amax(w.Wo, (size_t)H * I), a1 = amax(w.W1, (size_t)F * H), a2 = amax(w.W2, (size_t)H * F);
        worst = std::max(worst, std::max(std::max(std::max(aq, std::max(ak, av)), std::max(ae, ao)), std::max(a1, a2)));
        low(m1); low(m2); low(aq); low(ak); low(av); low(ae); low(ao); low(a1); low(a2);
        if (!kv.empty()) {
            // the k / v fold's kernel (round 6) splits two more activations as they are: q' = W_k,h^T (W_q,h n + b_q,h), an operand
            // of the logits -- |q'| <= (L1 norm of a row of W_k,h^T W_q,h) max|n| + |W_k,h^T b_q,h| -- and the rows of
            // G = dattn (W_o,h W_v,h), an operand of dA, whose input rows arrive scaled to a maximum below 32
            double qb = 0, gb = 0, qm = 0, om = 0;   // (qm, om: max|W_k,h^T W_q,h|, max|W_o,h W_v,h| -- the folded images)
            for (int r = 0; r < I; ++r) {   // r = h * 64 + e
                double l1 = 0, g1 = 0;
                for (int c = 0; c < H; ++c) {
                    const double sq = fabs(kv[l].Mq[(size_t)r * H + c]), so = fabs(kv[l].Wof[(size_t)c * I + r]);
                    l1 += sq; g1 += so;
                    qm = std::max(qm, sq); om = std::max(om, so);
                }
                qb = std::max(qb, l1 * m1 + fabs(kv[l].cq[r]));
                gb = std::max(gb, 32.0 * g1);
            }
            worst = std::max(worst, std::max(qb, gb));
            low(qm); low(om);
        }
    }
    char s[256] = "";
    if (!(worst < 1.6e4))
        snprintf(s, sizeof s, "dff: forward activations of this model may reach %.3g (> 1.6e4): the fp16 split engine is off, weight GEMMs run on the fp32 matrix pipe\n", worst);
    else if (least < 0x1p-12)
        snprintf(s, sizeof s, "dff: a weight matrix or LayerNorm row of this model is bounded by %.3g (< 2^-12): below the fp16 split engine's range, weight GEMMs run on the fp32 matrix pipe\n", least);
    return s;
}

// ---- one layer: folds (float64) and images ----
static PrepLayer prep_layer(const dff_config& cfg, const EmbedWeights& emb, const LayerWeights& w, const KvFold* kv, bool split,
                            bool small_split) {
    const int H = cfg.hidden, I = DFF_INNER, F = 4 * H, nfe = (int)emb.nfe;
    const int intr = cfg.use_intrinsic_coords, dist = cfg.use_distances, ab = cfg.use_abs_coords;
    const float *Wq = w.Wq, *bq = w.bq, *Wkv = w.Wkv, *bkv = w.bkv, *Wek = w.Wek, *Wo = w.Wo, *W1 = w.W1, *W2 = w.W2, *We = emb.We;
    // ---- fold edge_embedding into edges_to_kv (float64): W_c (512x3), b_c (512) ----
    // W_c3 (512x3): the intrinsic-coordinate columns (zero without them); cd (512): the distance column
    std::vector<double> Wc((size_t)I * 3, 0.0), cd(I, 0.0), bc(I);
    for (int r = 0; r < I; ++r) {
        double s0 = 0, s1 = 0, s2 = 0, sd = 0, sb = 0;
        for (int c = 0; c < H; ++c) {
            const double e = Wek[(size_t)r * H + c];
            if (intr) { s0 += e * We[c * nfe + 0]; s1 += e * We[c * nfe + 1]; s2 += e * We[c * nfe + 2]; }
            if (dist) sd += e * We[c * nfe + 3 * intr];
            sb += e * emb.be[c];
        }
        Wc[r * 3 + 0] = s0; Wc[r * 3 + 1] = s1; Wc[r * 3 + 2] = s2;
        cd[r] = sd;
        bc[r] = sb + w.bek[r];
    }
    // distance term: s_ih = c_h . q_ih -> W_s (8xH), b_s (8) ; D_ih feeds the output through w_od,h = W_o,h c_h (Hx8)
    std::vector<double> Wsd((size_t)8 * H, 0.0), bsd(8, 0.0), Wod((size_t)H * 8, 0.0);
    for (int h = 0; h < DFF_HEADS; ++h) {
        for (int c = 0; c < H; ++c) {
            double s = 0, t = 0;
            for (int dd = 0; dd < DFF_DH; ++dd) {
                s += cd[h * 64 + dd] * Wq[(size_t)(h * 64 + dd) * H + c];
                t += (double)Wo[(size_t)c * I + h * 64 + dd] * cd[h * 64 + dd];
            }
            Wsd[(size_t)h * H + c] = s;
            Wod[(size_t)c * 8 + h] = t;
        }
        double s = 0;
        for (int dd = 0; dd < DFF_DH; ++dd) s += cd[h * 64 + dd] * bq[h * 64 + dd];
        bsd[h] = s;
    }
    // W_u (24xH), b_u (24): u_ih = W_c,h^T q_ih ; W_oc (Hx24) = W_o,h W_c,h ; b_o' = b_o + W_o b_c
    std::vector<double> Wu((size_t)24 * H, 0.0), bu(24, 0.0), Woc((size_t)H * 24, 0.0), bof(H);
    for (int h = 0; h < DFF_HEADS; ++h)
        for (int cc = 0; cc < 3; ++cc) {
            for (int c = 0; c < H; ++c) {
                double s = 0;
                for (int dd = 0; dd < DFF_DH; ++dd) s += Wc[(h * 64 + dd) * 3 + cc] * Wq[(size_t)(h * 64 + dd) * H + c];
                Wu[(size_t)(3 * h + cc) * H + c] = s;
            }
            double s = 0;
            for (int dd = 0; dd < DFF_DH; ++dd) s += Wc[(h * 64 + dd) * 3 + cc] * bq[h * 64 + dd];
            bu[3 * h + cc] = s;
            for (int c = 0; c < H; ++c) {
                double t = 0;
                for (int dd = 0; dd < DFF_DH; ++dd) t += (double)Wo[(size_t)c * I + h * 64 + dd] * Wc[(h * 64 + dd) * 3 + cc];
                Woc[(size_t)c * 24 + 3 * h + cc] = t;
            }
        }
    for (int c = 0; c < H; ++c) {
        double s = w.bo[c];
        for (int r = 0; r < I; ++r) s += (double)Wo[(size_t)c * I + r] * bc[r];
        bof[c] = s;
    }
    // ---- H == head dimension: W_k folded into W_q and W_v into W_o (kv_fold) ----
    // The kernels keep their [q | u | k | v] layout: the k and v blocks of the images become identities (exactly
    // representable, so k = v = n bit for bit) and the <= 16-row kernel skips them altogether.  u, s, W_oc, W_od above
    // are built from the ORIGINAL q and W_o: the edge terms are untouched.
    const bool fold = kv != nullptr;
    if (fold)
        for (int c = 0; c < H; ++c) {
            double sbv = 0;
            for (int r = 0; r < I; ++r) sbv += (double)Wo[(size_t)c * I + r] * bkv[I + r];
            bof[c] += sbv;
        }
    PrepLayer p;
    auto copy = [](const float* a, size_t n) { return std::vector<float>(a, a + n); };
    p.ln1_g = copy(w.ln1g, H); p.ln1_b = copy(w.ln1b, H);
    p.g1 = copy(w.g1, 3 * H);
    p.ln2_g = copy(w.ln2g, H); p.ln2_b = copy(w.ln2b, H);
    p.b1 = copy(w.b1, F);
    p.b2 = copy(w.b2, H);
    p.g2 = copy(w.g2, 3 * H);
    p.bo.resize(H);
    for (int c = 0; c < H; ++c) p.bo[c] = (float)bof[c];
    // extended-head images: column e of head h: [0,64) q, [64,67) u, [67,80) 0, [80,144) k, [144,208) v
    auto wqkvx = [&](int col, int c) -> double {
        const int h = col / 208, e = col % 208;
        if (e < 64) return fold ? kv->Mq[(size_t)(h * 64 + e) * H + c] : (double)Wq[(size_t)(h * 64 + e) * H + c];
        if (e < 80) return e < 67 ? Wu[(size_t)(3 * h + e - 64) * H + c] : e == 67 ? Wsd[(size_t)h * H + c] : 0.0;
        if (fold) return (e < 144 ? e - 80 : e - 144) == c ? 1.0 : 0.0;
        if (e < 144) return Wkv[(size_t)(h * 64 + e - 80) * H + c];
        return Wkv[(size_t)(I + h * 64 + e - 144) * H + c];
    };
    p.bqkvx.assign(8 * 208, 0.f);
    for (int col = 0; col < 8 * 208; ++col) {
        const int h = col / 208, e = col % 208;
        p.bqkvx[col] = e < 64 ? (fold ? (float)kv->cq[h * 64 + e] : bq[h * 64 + e]) : e < 67 ? (float)bu[3 * h + e - 64] : e == 67 ? (float)bsd[h]
                       : e < 80 ? 0.f : fold ? 0.f : e < 144 ? bkv[h * 64 + e - 80] : bkv[I + h * 64 + e - 144];
    }
    // output projection with the xrel rows: row e of head h: [0,64) W_o[:, h*64+e], [64,67) W_oc[:, 3h+e-64]
    auto wox = [&](int krow, int c) -> double {
        const int h = krow / 80, e = krow % 80;
        if (e < 64) return fold ? kv->Wof[(size_t)c * I + h * 64 + e] : (double)Wo[(size_t)c * I + h * 64 + e];
        return e < 67 ? Woc[(size_t)c * 24 + 3 * h + e - 64] : e == 67 ? Wod[(size_t)c * 8 + h] : 0.0;
    };
    // the eight weight-GEMM operands, (k, n) -> weight, in both orientations (forward / VJP); every image below is packed from them
    const Operand oW1{H, F, [&](int k, int n) { return (double)W1[(size_t)n * H + k]; }};
    const Operand oW2{F, H, [&](int k, int n) { return (double)W2[(size_t)n * F + k]; }};
    const Operand oW2T{H, F, [&](int k, int n) { return (double)W2[(size_t)k * F + n]; }};
    const Operand oW1T{F, H, [&](int k, int n) { return (double)W1[(size_t)k * H + n]; }};
    const Operand oQkvx{H, 8 * 208, [&](int k, int n) { return wqkvx(n, k); }};
    const Operand oWoxT{H, 8 * 80, [&](int k, int n) { return wox(n, k); }};
    const Operand oWox{8 * 80, H, [&](int k, int n) { return wox(k, n); }};
    const Operand oQkvxT{8 * 208, H, [&](int k, int n) { return wqkvx(k, n); }};
    // the fp16 engines take the REGULAR rows of the last two -- the 64 of every head of [W_o ; W_oc], the 192 [q | k | v] of every head
    // of QKV_ext^T -- (the extension rows stay on the fp32 images: an fp32 k-step)
    const Operand oWoxR{8 * 64, H, [&](int k, int n) { return wox(k / 64 * 80 + k % 64, n); }};
    const Operand oQkvxTR{8 * 192, H, [&](int k, int n) { return wqkvx(k / 192 * 208 + (k % 192 < 64 ? k % 192 : k % 192 + 16), n); }};
    // fold_kv on the shipped input branch: the <= 16-row kernel's FOLD variant streams [q' | u] (5 tiles per head) and
    // back-projects dQ only (2 k-blocks per head); k = v = LayerNorm output never goes through a GEMM there
    const bool sfold = fold && intr && !dist && !ab;
    const Operand oQU{H, 8 * 80, [&](int k, int n) { return wqkvx(n / 80 * 208 + n % 80, k); }};
    const Operand oQT{8 * 64, H, [&](int k, int n) { return wqkvx(k / 64 * 208 + k % 64, n); }};
    const struct {
        std::vector<float> PrepLayer::*p; const Operand* full; int xper;       // fp32 image
        std::vector<uint32_t> PrepLayer::*s; const Operand* reg;               // fp16 image of the <= 64-row kernel
        std::vector<uint32_t> PrepLayer::*u; const Operand* unit; bool tall;   // unit image of the <= 16-row kernel
    } images[] = {
        {&PrepLayer::W1_p, &oW1, 0, &PrepLayer::W1_s, &oW1, &PrepLayer::W1_w, &oW1, false},
        {&PrepLayer::W2_p, &oW2, 0, &PrepLayer::W2_s, &oW2, &PrepLayer::W2_t, &oW2, true},
        {&PrepLayer::W2T_p, &oW2T, 0, &PrepLayer::W2T_s, &oW2T, &PrepLayer::W2T_w, &oW2T, false},
        {&PrepLayer::W1T_p, &oW1T, 0, &PrepLayer::W1T_s, &oW1T, &PrepLayer::W1T_t, &oW1T, true},
        {&PrepLayer::Wqkvx_p, &oQkvx, 0, &PrepLayer::Wqkvx_s, &oQkvx, &PrepLayer::Wqkvx_w, sfold ? &oQU : &oQkvx, false},
        {&PrepLayer::WoxT_p, &oWoxT, 0, &PrepLayer::WoxT_s, &oWoxT, &PrepLayer::WoxT_w, &oWoxT, false},
        {&PrepLayer::Wox_p, &oWox, 5, &PrepLayer::Wox_s, &oWoxR, &PrepLayer::Wox_t, &oWoxR, true},
        {&PrepLayer::WqkvxT_p, &oQkvxT, 13, &PrepLayer::WqkvxT_s, &oQkvxTR, &PrepLayer::WqkvxT_t, sfold ? &oQT : &oQkvxTR, true},
    };
    for (const auto& t : images) {
        p.*t.p = pack_b(*t.full, t.xper);
        if (split) p.*t.s = pack_b_split_f16(*t.reg);
        if (small_split) p.*t.u = pack_units_f16(*t.unit, t.tall);
    }
    return p;
}

DffPrep dff_prepare(const dff_config& cfg, const float* w, bool want_split, bool want_fold, bool small_spw) {
    const int H = cfg.hidden, L = cfg.n_layers;
    Cursor cur{w};
    const EmbedWeights emb = cut_embed(cur, cfg);
    std::vector<LayerWeights> layers;
    for (int l = 0; l < L; ++l) layers.push_back(cut_layer(cur, H));
    DffPrep out;
    // (the <= 16-row FOLD kernel keeps a model's forward activations in LDS / registers: built for <= 3 layers, which is
    // every shipped configuration; a deeper hidden-64 model runs the unfolded kernels)
    const bool can_fold = H == DFF_DH && L <= 3;
    out.fold_kv = can_fold && want_fold;
    // the fold products, once: the guard bounds what the FOLD kernels would split whether or not the fold is applied
    std::vector<KvFold> kv;
    if (can_fold && (want_split || out.fold_kv))
        for (const LayerWeights& l : layers) kv.push_back(kv_fold(l));
    if (want_split) out.note = range_guard(layers, H, kv);
    out.split = want_split && out.note.empty();
    out.small_split = out.split && small_spw;
    const int NI = (int)emb.NI, dec = (int)emb.dec;
    out.WnT.resize((size_t)NI * H);
    for (int c = 0; c < H; ++c)
        for (int i = 0; i < NI; ++i) out.WnT[(size_t)i * H + c] = emb.Wn[(size_t)c * NI + i];
    out.bn.assign(emb.bn, emb.bn + H);
    out.wdec.assign(emb.wd, emb.wd + (size_t)dec * H);
    out.bdec = emb.bd[0];
    for (int c = 0; c < 3; ++c) out.bdec3[c] = dec == 3 ? emb.bd[c] : 0.f;
    for (int l = 0; l < L; ++l)
        out.layer.push_back(prep_layer(cfg, emb, layers[l], out.fold_kv ? &kv[l] : nullptr, out.split, out.small_split));
    build_schedule(cfg.timesteps, out.sched);
    return out;
}
}   // namespace dff_prep
