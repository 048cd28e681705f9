/*
 * dff.h -- C ABI of the MI355X-native denoising-force-field sampler (libdff_amd.so).
 *
 * The reference (microsoft/two-for-one-diffusion) is pure Python/PyTorch and has no FFI; the
 * seams this library sits behind are its Python call signatures.  Each
 * entry point below names the reference interface it replaces.  Plain pointers and sizes only:
 * no torch types cross this boundary.  The host-side mirror of the reference classes that
 * binds these symbols (ctypes) is two-for-one-diffusion_amd/{binding,score,ddpm,langevin}.py;
 * INTEGRATION.md shows the stub a reference maintainer would add.
 *
 * Conventions
 *   - every *_dev pointer is device memory on the model's GPU, fp32, row-major, owned by the
 *     caller (e.g. torch-ROCm tensors); the library owns only its packed weights and scratch;
 *   - calls enqueue on `stream` (a hipStream_t, NULL = default stream) and do not synchronise: every kernel, memset and
 *     copy of a call is ordered on `stream` and on no other, and the call returns without waiting for the device
 *     (tests/test_stream_order.py holds every entry point to both).  The calls that DO block the host say so below:
 *     dff_model_create, the status calls, the dff_debug_* calls, and the FIRST ("cold") dff_score / dff_langevin_run /
 *     dff_ddpm_run / dff_denoise_loss of a model at a new batch size, group size, kernel variant or noise level -- it grows the
 *     model's scratch (hipFree / hipMalloc) and, in the sampling loops, builds the layer-0 table of that noise level (allocations,
 *     a host-to-device copy, hipStreamSynchronize(stream) between its chunks).  The identical call repeated never blocks;
 *   - ONE model on TWO streams at once is not supported: its scratch stash, layer-0 tables and flag words are shared by all
 *     of its launches, and only the order of one stream keeps them apart.  Different models, and the stateless dff_pwd_* /
 *     dff_struct_* / dff_tica_* / dff_kmeans_* / dff_transition_counts / dff_rmsd_* calls, may run on different streams at
 *     once (the caller's workspace must not be shared between them);
 *   - return 0 on success, a DFF_E* / hipError_t-derived code otherwise; dff_last_error()
 *     gives the message.  No exceptions cross the ABI;
 *   - one handle per device; not thread-safe per handle (the reference is single-threaded per
 *     replica, sample.py:176-190).
 */
#ifndef DFF_H
#define DFF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DFF_OK 0
#define DFF_EINVAL 1      /* bad argument / unsupported configuration */
#define DFF_EHIP 2        /* a HIP runtime call failed (see dff_last_error) */
#define DFF_ENOMEM 3

#define DFF_MAX_BEADS 64      /* array bound of the ABI structs */
#define DFF_MAX_BEADS_LDS 61  /* largest n_beads dff_model_create accepts: what the kernels' 160 KB of LDS hold (hidden 128) */

typedef struct dff_model dff_model; /* opaque */

/* Hyper-parameters of GraphTransformer.__init__ as sample.py passes them
 * (models/__init__.py:4-15, models/graph_transformer.py:23-75).  Every combination of the 0/1 input
 * flags is implemented: use_intrinsic_coords (edge features x_j - x_i), use_distances (edge feature
 * |x_j - x_i|^2), use_abs_coords (node features include x) -- :53-58,99-102,116-140 -- and
 * conservative (1: forces = -dE/dx through the hand-written VJP; 0: the force head of :62-65,112-113,
 * node_decoder = Linear(H,3), forces = its output, no energy).  All shipped checkpoints are
 * (1, 0, 0, conservative 1) and run the specialised kernels; main_train.py's defaults (0, 1, 1) and the
 * other combinations run the general ("gen") variants of the <= 64-row kernel. */
typedef struct {
    int32_t n_beads;              /* num_beads, 2..DFF_MAX_BEADS_LDS */
    int32_t hidden;               /* hidden_features_gnn: 64, 96, 128 (n_beads <= 61 with 128, <= 32 otherwise) or 256 (<= 32 beads) */
    int32_t n_layers;             /* num_layers_gnn, 1..8 */
    int32_t timesteps;            /* diffusion_steps (GaussianDiffusion timesteps), e.g. 1000 */
    int32_t use_intrinsic_coords; /* 0 / 1 */
    int32_t use_distances;        /* 0 / 1 */
    int32_t use_abs_coords;       /* 0 / 1 */
    int32_t conservative;         /* 1: forces = -dE/dx ; 0: forces = node_decoder(nodes) */
} dff_config;

/* Number of fp32 values dff_model_create expects for this config. */
size_t dff_weight_count(const dff_config* cfg);

/* Build a model from the GraphTransformer parameters, given as ONE flat host fp32 array in the
 * reference's state_dict() order: node_embedding.{weight (H, N+1+3*abs), bias},
 * edge_embedding.{weight (H, 3*intrinsic+distances, or 1 if neither), bias}, node_decoder.{weight (D,H), bias (D)} with D = 1
 * (conservative) or 3, then per layer
 * l: attn to_q.{weight (512,H), bias}, to_kv.{weight (1024,H), bias}, edges_to_kv.{weight
 * (512,H), bias}, to_out.{weight (H,512), bias}, norm.{weight, bias}, gate proj.0.weight
 * (1,3H), ff fn.0.{weight (4H,H), bias}, fn.2.{weight (H,4H), bias}, norm.{weight, bias}, gate
 * proj.0.weight (1,3H).  Replaces get_model + load_state_dict (sample.py:142-167): the
 * library folds edge_embedding into edges_to_kv, packs the GEMM operands for MFMA and builds
 * the cosine schedule tables of GaussianDiffusion.__init__ (models/ddpm.py:45-99). */
int dff_model_create(const dff_config* cfg, const float* weights_host, size_t n_weights,
                     int device, dff_model** out);
void dff_model_destroy(dff_model* m);

/* GaussianDiffusion schedule buffer `which` (models/ddpm.py:61-99) copied to out_host[timesteps]:
 * 0 betas, 1 alphas_cumprod, 2 alphas_cumprod_prev, 3 sqrt_alphas_cumprod,
 * 4 sqrt_one_minus_alphas_cumprod, 5 log_one_minus_alphas_cumprod, 6 sqrt_recip_alphas_cumprod,
 * 7 sqrt_recipm1_alphas_cumprod, 8 posterior_variance, 9 posterior_log_variance_clipped,
 * 10 posterior_mean_coef1, 11 posterior_mean_coef2. */
int dff_schedule(const dff_model* m, int which, float* out_host);

/* The score op: GraphTransformer.forward (models/graph_transformer.py:77-114) including
 * compute_forces (:143-159).  x_dev (batch,N,3) need not be centred; tnorm_dev (batch) is the
 * normalised time t/T per sample; force_dev (batch,N,3) receives -d(sum E)/d(x_centred);
 * energy_dev (batch,N), optional, receives the per-bead energies (return_energy=True). */
int dff_score(dff_model* m, const float* x_dev, const float* tnorm_dev, int batch,
              float* force_dev, float* energy_dev, void* stream);

/* Langevin.simulate driven by ForcesWrapper (dynamics/langevin_cgnet.py:686-792,447-500;
 * dynamics/langevin.py:75-92), n_steps steps in ONE launch.  Scalars are what
 * LangevinDiffusion.__init__ / Langevin._input_option_checks compute on the host
 * (langevin.py:131-184, langevin_cgnet.py:329-330,343). */
typedef struct {
    float t_norm;      /* noise level t / diffusion_steps (langevin.py:68) */
    float force_scale; /* 1 / (kbt_inv * sqrt_one_minus_alphas_cumprod[t]) (langevin.py:79-87) */
    float dt;          /* time step */
    float vscale;      /* exp(-friction dt); ignored when overdamped */
    float noisescale;  /* sqrt(1 - vscale^2); ignored when overdamped */
    float beta;        /* kb_inv / temp_sim */
    float dtau;        /* diffusion * dt, overdamped only (langevin_cgnet.py:343) */
    int32_t overdamped;            /* 1: friction is None -> Brownian step (:481-500) */
    float masses[DFF_MAX_BEADS];   /* per-bead masses (first n_beads used) */
} dff_langevin_params;

/* x_dev (n_traj,N,3) in/out, normalised units (init_mol / norm_factor); v_dev (n_traj,N,3)
 * in/out (ignored when overdamped).  noise_dev: (n_steps,n_traj,N,3) standard normals to use
 * (parity mode), or NULL to draw them in-kernel from Philox4x32-10 keyed by (seed; trajectory
 * traj_offset+i, step step_offset+s, bead).  Every save_interval steps the UN-centred x_new is
 * written to frames_dev (n_steps/save_interval, n_traj, N, 3) and 0.5 sum m v^2 to ke_dev
 * (n_steps/save_interval, n_traj) -- the layout of Langevin.simulated_coords /
 * .kinetic_energies before _swap_and_export (langevin_cgnet.py:410-425,502-542).  Either may be
 * NULL.  n_steps must be a multiple of save_interval when frames_dev != NULL.
 * In-kernel noise: the draw for (trajectory, step, bead, component) is the Philox4x32-10 block of key = (seed low word, seed
 * high word), counter = (index low word, (index >> 32) ^ (bead << 8), step low word, step high word), index = traj_offset + i,
 * step = step_offset + s, through a Box-Muller: components 0 / 1 = r(w0) cos / sin(2 pi u(w1)), component 2 = r(w2) cos(2 pi u(w3)),
 * u(w) = (float(w) + 0.5) 2^-32, r(w) = sqrt(-2 ln u(w)) (oracle/noise.py is the host reference; tests/test_noise_stream.py
 * holds every kernel variant to it).  It does not depend on how a batch is sharded, chunked, grouped or on the kernel variant.
 * LIMIT: the bead index shares counter word 1 with bits 32.. of the trajectory index, so with noise_dev == NULL
 * traj_offset + n_traj must not exceed 2^40 (DFF_EINVAL otherwise: beyond it two trajectories would share draws).
 * Steps in use: step_offset + s here; the level t (0 .. T - 1) and 0xFFFFFFFF (the prior) in dff_ddpm_run; 0xFFFFFFFE00000000 | draw
 * for the forward process (dff_q_sample / dff_denoise_loss), reserved for it: a step_offset that high would alias those draws. */
int dff_langevin_run(dff_model* m, const dff_langevin_params* p, int n_traj, float* x_dev,
                     float* v_dev, const float* noise_dev, uint64_t seed, uint64_t traj_offset,
                     uint64_t step_offset, int n_steps, int save_interval, float* frames_dev,
                     float* ke_dev, void* stream);

/* GaussianDiffusion.p_sample_loop body (models/ddpm.py:195-254): reverse steps t_start,
 * t_start-1, ..., t_end (inclusive) in ONE launch, each followed by the +-1000 clamp and
 * centring.  x_dev (batch,N,3) in/out in normalised units; if init_prior != 0 x is first set to
 * center_zero(randn) in-kernel (ddpm.py:242).  noise_dev: (t_start-t_end+1,batch,N,3) draws for
 * randn_like (ddpm.py:228), or NULL for in-kernel Philox keyed by (seed; sample
 * sample_offset+i, t) as dff_langevin_run keys its draws, with step = t for the reverse step of level t and step = 0xFFFFFFFF
 * for the prior; likewise sample_offset + batch must not exceed 2^40 when noise_dev == NULL (DFF_EINVAL otherwise).
 * *clamp_flag_dev (optional) is set to 1 if any coordinate was clamped
 * (the reference's "Large molecule encountered" warning, ddpm.py:248-250). */
int dff_ddpm_run(dff_model* m, int batch, float* x_dev, const float* noise_dev, uint64_t seed,
                 uint64_t sample_offset, int t_start, int t_end, int init_prior,
                 int* clamp_flag_dev, void* stream);

/* ---- the forward process and its loss (csrc/dff_loss.hip) ----
 * GaussianDiffusion.q_sample followed by the center_zero of p_losses (models/ddpm.py:265-274, 292-296):
 *   xt[b] = center_zero(sqrt_alphas_cumprod[t_b] x0[b] + sqrt_one_minus_alphas_cumprod[t_b] center_zero(z[b])),
 * fp32 on the model's own schedule tables, and tnorm[b] = float(t_b) / float(T) (tnorm_dev may be NULL).  x0_dev (batch,N,3)
 * is used as given: centring it and dividing by norm_factor are the caller's job, as in GaussianDiffusion.forward.
 * t_dev (batch) int32 levels, 0 <= t_b < T; nothing is read back to check them: a level outside the range gives NaN in that
 * sample's outputs (and only there).  z: noise_dev (batch,N,3), or NULL for in-kernel Philox draws keyed as
 * dff_langevin_run keys its draws with item = sample_offset + b and
 *   step = 0xFFFFFFFE00000000 | draw
 * -- a step value RESERVED for the forward process: the DDPM loop uses steps 0 .. T - 1 and 0xFFFFFFFF, Langevin
 * step_offset + s; a Langevin run whose step_offset reaches 0xFFFFFFFE00000000 would alias it.  `draw` noises one structure
 * several times independently.  The same 2^40 item limit applies: sample_offset + batch must not exceed 2^40 when
 * noise_dev == NULL (DFF_EINVAL otherwise).  The draws do not depend on how a batch is split over calls. */
int dff_q_sample(dff_model* m, const float* x0_dev, const int32_t* t_dev, int batch,
                 const float* noise_dev, uint64_t seed, uint64_t sample_offset, uint32_t draw,
                 float* xt_dev, float* tnorm_dev, void* stream);

/* Bytes of device workspace dff_denoise_loss needs for `batch` samples: x_t, tnorm and the model output of one pass of at
 * most 16384 samples plus 256 partial sums -- bounded, whatever the batch; -1 on bad arguments. */
long long dff_denoise_workspace_bytes(const dff_model* m, int batch);
/* GaussianDiffusion.p_losses for objective = "pred_noise" (models/ddpm.py:288-315) in one call: dff_q_sample into the workspace,
 * the score op on the launch path of dff_score (every configuration dff_score accepts, the same kernels), then
 *   loss_dev[b] = mean over the 3 N entries of |d| (loss_type 1, l1) or d^2 (2, l2),  d = center_zero(model_out[b]) - center_zero(z[b])
 * -- the mean of row b of the reference's reduce(loss, "b ... -> b (...)", "mean"), whose mean over b p_losses returns; the
 * centring, d and the mean are taken in fp64 and rounded to fp32 once.  With noise_dev == NULL the target is drawn again from Philox where it is used: the noise never exists in memory.
 * A level outside 0 .. T - 1 gives loss_dev[b] = NaN.
 * total_dev (2 doubles, may be NULL) is ADDED to: total[0] += the fp64 sum of loss_dev, total[1] += batch (a non-finite loss
 * adds to both).  The sum is a two-stage reduction in a fixed order without floating-point atomics: bit-identical from call to
 * call, as dff_kmeans_step's.  Results do not depend on dff_debug_max_workgroups.
 * xt_out_dev / model_out_dev (batch,N,3), optional: copies of x_t and of the score output before its centring.
 * workspace_dev: >= dff_denoise_workspace_bytes(m, batch) bytes, 8-byte aligned; a batch beyond one pass runs as consecutive
 * passes over it. */
int dff_denoise_loss(dff_model* m, const float* x0_dev, const int32_t* t_dev, int batch,
                     const float* noise_dev, uint64_t seed, uint64_t sample_offset, uint32_t draw,
                     int loss_type /* 1 = l1, 2 = l2 */, float* loss_dev /* (batch) */,
                     double* total_dev /* (2), may be NULL */, float* xt_out_dev, float* model_out_dev /* may be NULL */,
                     void* workspace_dev, size_t workspace_bytes, void* stream);

/* Sticky status word of everything this model has launched so far (synchronises the device).  0 = fine.  Bit 0: a launch
 * of a two-workgroups-per-protein kernel variant (chosen automatically for batches that would leave half the CUs idle, see
 * dff_debug_pair) gave up waiting for a partner workgroup -- possible only when the GPU is shared with another process or
 * partitioned below the CU count the driver reports; the results of that launch are invalid.  The samplers call this at
 * their host synchronisation points (end of LangevinDiffusion.simulate, GaussianDiffusion.check_clamp, the CLI) and raise;
 * once the host has seen the word, further launches on the same model run the one-workgroup-per-protein kernels (round 6;
 * they used to be refused with DFF_EHIP) until dff_model_status_clear re-arms; one queued before that
 * leaves at kernel entry (the word is read on the device) with its OUTPUTS set to NaN (forces / energies, frames / kinetic
 * energies, samples; the Langevin state x, v is left alone), so nothing runs on top of invalid results and a caller that
 * never checks cannot mistake an unwritten buffer for forces.  The entry points
 * themselves never read it: they only enqueue on the caller's stream (round 4; they used to synchronise the device before
 * every two-workgroups launch).  The reference has no counterpart (one process, one kernel per op).  NOTE: which variant runs depends on the per-call batch (<= n_CUs / 2 proteins), and the two variants sum
 * in different orders: trajectories are bit-reproducible for a fixed per-rank batch, not across batch splits that cross
 * that threshold. */
int dff_model_status(dff_model* m, unsigned* status);
/* Clear the sticky word (synchronises the device): re-arms the two-workgroups variants after the caller has dealt with a
 * reported failure (e.g. the co-tenant that held the CUs is gone).  dff_debug_pair(m, 0) clears it as well (whether or not
 * the host has read it yet). */
int dff_model_status_clear(dff_model* m);

/* ---- introspection / debugging (used by tests and bench.py, not by samplers) ---- */

/* Proteins handled per workgroup for this model (0 = choose automatically from batch). */
int dff_set_group(dff_model* m, int proteins_per_workgroup);
/* Debugging: on != 0 disables the rows<=16 fast-path kernel so the generic kernel runs. */
int dff_debug_force_generic(dff_model* m, int on);
/* Debugging: waves per workgroup of the rows<=16 kernel: 0 auto (8 where it applies), 4 or 8.  A non-zero value also keeps
 * hidden-96 / 128 models on that kernel (by default they run the one-row-tile split variant of the <= 64-row kernel, which is faster). */
int dff_debug_small_waves(dff_model* m, int waves);
/* Workgroups per kernel launch (default 2048).  Proteins are independent, so a batch that needs more
 * workgroups runs as consecutive launches over one bounded scratch "stash" (n x stash slot) instead
 * of a scratch allocation that grows with the batch.  Results do not depend on the limit. */
int dff_debug_max_workgroups(dff_model* m, int n);
/* Debugging: on == 0 makes the sampling loops recompute layer 0 every step instead of reading the
 * precomputed per-noise-level table of layer-0 inputs (results are bit-identical either way). */
int dff_debug_l0_table(dff_model* m, int on);
/* Debugging: on == 2 = on, and the exchanges always run the agent-scope protocol of a pair whose blocks sit on different XCDs
 * (never observed: blocks b and b + 8 share one; the kernel checks at run time and takes an L2-local path when they do).
 * on == 3 = on, with partners placed on ADJACENT blocks (b, b + 1): under the hardware's round-robin placement they sit on
 * different XCDs, so the run-time check itself selects the agent-scope protocol on pairs that really span two L2s.
 * on == 0 never splits a protein over two workgroups (the PAIR variants of the <= 64-row kernel, chosen
 * automatically when one workgroup per protein would leave at least half the CUs idle, e.g. protein G at 128 per GPU). */
int dff_debug_pair(dff_model* m, int on);
/* dff_model_status for tests: *status = the sticky word, which is then CLEARED.  Synchronises the device. */
int dff_debug_pair_status(dff_model* m, int* status);
/* Tests: overwrite the sticky word ON THE DEVICE as a kernel that lost its partner would (the host's cached copy is not
 * touched), to exercise the failure path: queued two-workgroups launches leave at entry, dff_model_status reports. */
int dff_debug_poke_status(dff_model* m, unsigned word);
/* Name of the kernel the last call launched, grid size and dynamic LDS bytes. */
int dff_last_launch(const dff_model* m, const char** kernel_name, int* grid, int* lds_bytes);
/* Everything kernel selection reads of a model besides its dff_config: the engines weight preparation chose, the device's
 * CU count, the debug knobs above, the sticky word as the host last read it, and the two environment opt-ins. */
typedef struct {
    int32_t split, small_split, fold_kv;   /* fp16 images exist; ... also for the <= 16-row kernel; k / v folded (hidden 64) */
    int32_t n_cus;                         /* hipDeviceAttributeMultiprocessorCount */
    int32_t group_override, small_waves, max_wgs, force_generic, l0_off, pair_off;   /* dff_set_group, dff_debug_* */
    int32_t sticky;                        /* dff_model_status word the host has seen */
    int32_t small_pair, small_h96;         /* DFF_SMALL_PAIR=1 (read at every launch), DFF_SMALL_H96=1 (once per process) */
} dff_dispatch;
/* What a call of `mode` (0 dff_score, 1 dff_langevin_run, 2 dff_ddpm_run) over `batch` proteins launches. */
typedef struct {
    const char* kernel;                    /* static string, as dff_last_launch reports it */
    int32_t G;                             /* proteins per workgroup */
    int32_t workgroups, launches;          /* in all, over `launches` consecutive kernel launches */
    int32_t last_grid;                     /* workgroups of the last launch: the grid dff_last_launch reports */
    int32_t lds_bytes, threads, pair;      /* dynamic LDS, threads per workgroup, 1: two workgroups per protein */
    int32_t table;                         /* layer-0 table: 0 none, 1 one entry (Langevin), 2 one entry per level (DDPM) */
    const char* table_kernel;              /* the kernel that builds it ("" when table == 0) */
} dff_launch_plan;
/* Host only, for tests: the model's dff_dispatch as the next launch would see it (the environment opt-ins read now).
 * No device access, no synchronisation. */
int dff_debug_dispatch(const dff_model* m, dff_dispatch* out);
/* Host only, for tests, no GPU needed: the launch plan of a model of this config and dispatch -- the function every
 * launch goes through, without a handle.  cfg is checked as dff_model_create checks it. */
int dff_debug_plan_launch(const dff_config* cfg, const dff_dispatch* dispatch, int mode, int batch, dff_launch_plan* out);
/* Run one MFMA GEMM stage out(M,Nout) = A(M,K) W(K,Nout) through the same device routine and
 * weight packing the score kernel uses (M <= 64; K, Nout multiples of 16).  Host pointers. */
int dff_debug_gemm(int device, const float* A_host, const float* W_host, int M, int K, int Nout,
                   float* out_host);
/* Copy one stashed forward intermediate of the LAST dff_score call for sample `b`, layer `l`
 * to out_host: what 0 nodes_in (N,H), 1 attn_out (N,H), 2 ff (N,H), 3 gelu'(h_pre) (N,4H; what the backward needs),
 * 4 q (N,512), 5 k (N,512), 6 v (N,512), 7 P (8,N,N), 8 u (N,32). */
int dff_debug_stash(dff_model* m, int b, int layer, int what, float* out_host, size_t n);

/* Per-stage cycle accounting of workgroup 0 (s_memtime deltas accumulated at the stage
 * boundaries of the fused kernel): enable != 0 makes subsequent launches record; _read copies
 * the DFF_NPROF (=24) totals of the last launch (shader-clock cycles) to out_host. */
int dff_debug_profile(dff_model* m, int enable);
int dff_debug_profile_read(dff_model* m, unsigned long long* out_host);

/* ---- pairwise-distance (PWD) histograms for the Jensen-Shannon sample-quality metric ----
 * Replaces, for structures already resident on the GPU, evaluate/evaluators.py: get_pwd_triu_batch
 * (:934-948), the per-pair maximum (:239, :259) and the per-pair torch.histc (:241-247, :261-263) of
 * PwdEvaluator -- without materialising the (n, n_pairs) distance matrix.  Pairs are (i, j >= i+offset)
 * in torch.triu_indices order; distances and bin selection reproduce torch's float32 arithmetic, so
 * the counts equal the reference's.  The (n_pairs x bins) JS reduction stays on the host
 * (two-for-one-diffusion_amd/evaluate.py). */
int dff_pwd_num_pairs(int n_beads, int offset);
/* Non-finite input (both calls): a distance is NaN when a coordinate of either bead is NaN or both beads have the same
 * infinite coordinate, and +Inf when one coordinate is infinite or a squared difference overflows fp32 (finite
 * |x| >~ 1.8e19).  dff_pwd_max skips NaN distances -- the maximum is over the others, 0 if there is none -- and a +Inf
 * distance makes the pair's maximum +Inf.  dff_pwd_hist drops NaN and +Inf distances and counts the rest, so the pairs
 * of one call may have different totals.  Leaving such frames out whole is the caller's business (PwdEvaluator does). */
/* max_out_dev[p] = max over the n structures of d_p (0 when n == 0).  x_dev: (n, n_beads, 3) fp32. */
int dff_pwd_max(int device, const float* x_dev, long long n, int n_beads, int offset,
                float* max_out_dev, void* stream);
/* hist_dev[p * ld + b], b < nbins_dev[p]: number of structures whose d_p falls into bin b of
 * torch.histc(d_p, bins=nbins[p], min=0, max=hmax_dev[p]); the call zeroes hist_dev (n_pairs * ld)
 * first.  max_bins >= every nbins[p]; ld >= max_bins.
 * 1 <= max_bins <= 30719 (3071.9 Angstrom at the metric's 0.1 Angstrom bins): a pair's histogram row of max_bins | 1
 * slots must fit the 30720 slots a workgroup keeps in LDS; more is DFF_EINVAL.
 * The device arrays are not read on the host, so their contents are the caller's responsibility: every nbins_dev[p]
 * must lie in 1..max_bins (anything else is an error of the caller that the call cannot see: the kernel would write
 * outside the pair's LDS row) and every hmax_dev[p] must be finite and > 0. */
int dff_pwd_hist(int device, const float* x_dev, long long n, int n_beads, int offset,
                 const int32_t* nbins_dev, const float* hmax_dev, int max_bins, int ld,
                 uint32_t* hist_dev, void* stream);
/* The launch layout dff_pwd_hist takes for these arguments. */
typedef struct {
    int32_t n_pairs;
    int32_t tile_n;                        /* structures per LDS tile: 64 or 32 */
    int32_t pc_log2, npc;                  /* 1 << pc_log2 pair lanes per workgroup (0..8), npc pair chunks of that many */
    int32_t ldl;                           /* LDS row stride of a pair's histogram: max_bins | 1 */
    int32_t lds_bytes;                     /* dynamic LDS: tile + (1 << pc_log2) * ldl counters + 16 */
    long long chunk;                       /* structures per structure chunk, a multiple of 64 */
    long long chunks, chunks_rounded;      /* structure chunks that hold structures; rounded up to whole rounds of 8 */
    long long grid;                        /* workgroups: chunks_rounded * npc */
} dff_pwd_plan;
/* Host only, for tests, no GPU needed: the function dff_pwd_hist itself plans its launch with.  DFF_EINVAL where
 * dff_pwd_hist refuses the shape (n_beads, offset, max_bins). */
int dff_pwd_hist_plan(int n_beads, int offset, int max_bins, long long n, dff_pwd_plan* out);

/* ---- per-frame structure metrics of the reference's evaluators (csrc/dff_struct.hip) ----
 * Stateless, like dff_pwd_*: x_dev is (n, n_beads, 3) fp32 in Angstrom on the device, 4 <= n_beads <= 64, frames
 * independent.  Only per-frame results (and one N x N count matrix) are written; the histogram and divergence
 * reductions stay on the host (two-for-one-diffusion_amd/evaluate.py).  No synchronisation on the launch path. */
/* rmsd_dev[s] = minimum over proper rotations of the RMSD between frame s and ref_dev (N, 3), both centred on their
 * unweighted mean; fp64 accumulation, largest eigenvalue of Horn's 4x4 key matrix by cyclic Jacobi.  NaN for a frame
 * with any non-finite coordinate.
 * Replaces md.rmsd(traj, folded) * 10 with its valid_mask, evaluate/evaluators.py:656-662. */
int dff_struct_rmsd(int device, const float* x_dev, long long n, int n_beads, const float* ref_dev,
                    float* rmsd_dev, void* stream);
/* out_dev (n, N - 3): dihedral of beads (i, i+1, i+2, i+3) in radians, mdtraj's formula in fp32.
 * Replaces md.compute_dihedrals of evaluate/evaluators_CGflowmatching.py:30-36 (ala2: phi, psi) and of
 * get_tic_features, evaluate/evaluators.py:439-441. */
int dff_struct_dihedrals(int device, const float* x_dev, long long n, int n_beads, float* out_dev, void* stream);
/* F = (N - 3) + N (N - 1) / 2 TIC features per frame (0 for N < 4). */
int dff_struct_tic_num_features(int n_beads);
/* out_dev[s * k + c] = sum_f (feat_f(s) - mean_dev[f]) * coeff_dev[f * k + c], 1 <= k <= 8, fp64.  feat = the N - 3
 * dihedrals then the pair distances in torch.triu_indices(N, N, 1) order, fp32 and never stored.
 * Replaces self.tica(self.get_tic_features(xyz)), evaluate/evaluators.py:433-445, :460-461. */
int dff_struct_tic(int device, const float* x_dev, long long n, int n_beads, const double* mean_dev,
                   const double* coeff_dev, int k, double* out_dev, void* stream);
/* counts_dev (N, N), zeroed by the call: number of frames with d_ij < cutoff (torch.norm's fp32 distance), the
 * diagonal included.  If mismatch_dev != NULL (folded_dev required): mismatch_dev[s] = number of pairs j >= i + offset
 * whose contact differs from folded_dev (N x N, 0 / 1).
 * Replaces _get_samp_contacts(xyz).sum(0) and the per-frame BCE of _eval_bce_dynamics,
 * evaluate/evaluators.py:781-806, :829-859 (a 0 / 1 mismatch costs exactly 100 there). */
int dff_struct_contacts(int device, const float* x_dev, long long n, int n_beads, float cutoff,
                        const uint8_t* folded_dev, int offset, uint32_t* counts_dev, uint32_t* mismatch_dev,
                        void* stream);
/* out_dev (n, F) fp32: the TIC features of every frame, N - 3 dihedrals then the pair distances in
 * torch.triu_indices(N, N, 1) order -- bit for bit the values dff_struct_tic projects.
 * Replaces get_tic_features, evaluate/evaluators.py:433-445. */
int dff_struct_tic_features(int device, const float* x_dev, long long n, int n_beads, float* out_dev, void* stream);

/* ---- TICA fitting: lag-tau second moments of the TIC features (csrc/dff_tica.hip) ----
 * The GPU half of TICA(lagtime, dim).fit_transform(get_tic_features(sorted data)), evaluate/evaluators.py:384-420: the
 * running sums of deeptime's symmetrised covariance estimator.  The covariances and the decomposition stay on the host
 * (two-for-one-diffusion_amd/evaluate.py).
 * Bytes of device workspace dff_tica_moments needs for calls of up to n_frames_max frames; -1 on bad arguments. */
long long dff_tica_workspace_bytes(int n_beads, long long n_frames_max, int lagtime);
/* x_dev (n, N, 3) fp32 holds n_traj time-ordered trajectories back to back, lengths_host[i] frames each (sum = n).
 * With g_t = feat(t) - shift_dev (fp64, F = dff_struct_tic_num_features(N)) and a_t = 1 when t lies in the first
 * L_i - lagtime frames of its trajectory (pairs never cross a trajectory; L_i <= lagtime contributes nothing), the call
 * ADDS, in fp64 (products on the f64 matrix cores), to the device accumulators
 *   sx_dev (F) += sum a_t g_t,   sy_dev (F) += sum a_t g_{t+lag},
 *   m0_dev (F, F) += sum a_t (g_t g_t^T + g_{t+lag} g_{t+lag}^T),   mt_dev (F, F) += sum a_t (g_t g_{t+lag}^T + g_{t+lag} g_t^T),
 * the matrices row-major, upper triangle (i <= j) only: the lower triangle is not touched.  Consecutive calls stream
 * trajectories (deeptime's partial_fit).  Deterministic: bit-identical from call to call, no atomics.
 * workspace_dev: >= dff_tica_workspace_bytes(N, n, lagtime) bytes, 8-byte aligned (DFF_EINVAL otherwise: it holds the doubles
 * of the partial sums), contents irrelevant.  4 <= N <= 64, lagtime >= 1. */
int dff_tica_moments(int device, const float* x_dev, long long n, int n_beads, const long long* lengths_host, int n_traj,
                     int lagtime, const double* shift_dev, void* workspace_dev, size_t workspace_bytes, double* sx_dev,
                     double* sy_dev, double* m0_dev, double* mt_dev, void* stream);
/* Host only, for tests: the chunk plan dff_tica_moments follows for these lengths (chunk_pairs > 0 overrides the chunk
 * size C, <= 0 takes the one of n_beads).  Writes up to max_runs records of 6 values, one per run of consecutive pair starts:
 * (chunk, chunk's first frame f0, chunk's feature rows, chunk's pairs, run's first pair start - f0, run's pairs); returns
 * the number of runs, -1 on bad arguments. */
int dff_tica_debug_plan(int n_beads, const long long* lengths_host, int n_traj, int lagtime, long long chunk_pairs,
                        long long* out_host, int max_runs);

/* ---- states in TIC space and the transitions between them (csrc/dff_states.hip) ----
 * The "Dynamics" section of evaluate/evaluate_fastfolders.ipynb (cells 20-24) on the device.  Stateless like
 * dff_struct_*: device pointers, enqueued on `stream`, no synchronisation on the launch path; n == 0 is a valid no-op
 * (outputs that a call zeroes or overwrites are zeroed).
 * Assignment rule of both assigning calls: d2_c = sum_j (p_j - centre_cj)^2 in fp64 (one FMA per coordinate, in order);
 * the label is the centre of smallest d2, the lowest index among equals.  A point with a non-finite coordinate gets
 * label -1 and d2 = NaN.
 *
 * Frames -> state labels in one pass: the projection of dff_struct_tic (same features, same FMA order: proj_dev, when
 * given, is bit-identical to its output), then the nearest of the K centres centers_dev (K, k).  labels_dev (n);
 * proj_dev (n, k) and dist2_dev (n) may be NULL.  1 <= k <= 8, 1 <= K <= 64, 4 <= n_beads <= 64.
 * Replaces tic_evaluator.tica(get_tic_features(sampled_mol)) + MiniBatchKMeans(max_iter=0,
 * initial_centers=...).fit_transform of cell 22. */
int dff_struct_tic_assign(int device, const float* x_dev, long long n, int n_beads, const double* mean_dev,
                          const double* coeff_dev, int k, const double* centers_dev, int K, int32_t* labels_dev,
                          double* proj_dev, double* dist2_dev, void* stream);
/* Bytes of device workspace dff_kmeans_step needs for n points when it accumulates; -1 on bad arguments. */
long long dff_kmeans_workspace_bytes(long long n, int d, int K);
/* One Lloyd iteration over points pts_dev (n, d) fp64 already projected, 1 <= d <= 8, 1 <= K <= 64: labels_dev (n) and
 * dist2_dev (n) by the rule above, and -- OVERWRITTEN, over the points with finite coordinates -- sums_dev (K, d) the
 * per-cluster coordinate sums, counts_dev (K) the member counts, inertia_dev (1) the sum of the smallest d2.  Every
 * output may be NULL; with the three accumulators NULL the call only assigns and needs no workspace.  Deterministic:
 * per-workgroup partials in the workspace, added in a fixed order by a second stage, no floating-point atomics --
 * bit-identical from call to call.  The k-means the presets of cell 21 were "determined via".
 * workspace_dev: >= dff_kmeans_workspace_bytes(n, d, K) bytes when it accumulates, 8-byte aligned (DFF_EINVAL otherwise: the
 * partials are doubles), contents irrelevant. */
int dff_kmeans_step(int device, const double* pts_dev, long long n, int d, const double* centers_dev, int K,
                    int32_t* labels_dev, double* dist2_dev, double* sums_dev, uint64_t* counts_dev, double* inertia_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);
/* Sliding-window transition counts for n_lags lag times in one pass: counts_dev (n_lags, K, K), zeroed by the call;
 * counts[l][i][j] = number of t with labels[t] = i, labels[t + lags[l]] = j, t and t + lags[l] in the same trajectory.
 * labels_dev (n) holds n_traj trajectories back to back, lengths_host[i] frames each (sum = n), as dff_tica_moments
 * takes them; a pair with a label outside 0 .. K - 1 (the -1 of a non-finite frame) is skipped.  lags >= 1,
 * 1 <= n_lags <= 8, 1 <= K <= 64.  Integer counting: exact, the same from call to call.
 * Replaces TransitionCountEstimator.count("sliding", [assignments], lagtime=1) of cell 22 (one trajectory of n frames
 * is that call; the notebook hands it all simulations as one trajectory). */
int dff_transition_counts(int device, const int32_t* labels_dev, long long n, const long long* lengths_host, int n_traj,
                          const int32_t* lags_host, int n_lags, int K, uint64_t* counts_dev, void* stream);

/* ---- RMSD between two ensembles: nearest structure and dense matrix (csrc/dff_ensemble.hip) ----
 * Novelty (samples -> nearest training structure), coverage (held-out structures -> nearest sample) and diversity
 * (samples -> nearest other sample).  Stateless like dff_struct_*: x_dev (n, n_beads, 3) the queries and y_dev
 * (m, n_beads, 3) the candidates, fp32 in Angstrom on the device, 4 <= n_beads <= 64; enqueued on `stream`, no
 * synchronisation on the launch path; n == 0 is a valid no-op.
 * The distance of a pair is the quantity dff_struct_rmsd computes: the minimum over PROPER rotations (a mirror image does
 * not match) of the RMSD of the two frames, each centred on its unweighted mean in fp64; the 3 x 3 correlation in fp64
 * on the matrix cores, the largest eigenvalue of Horn's 4 x 4 key matrix by cyclic Jacobi, sqrt(max(msd, 0)) rounded to
 * fp32 once.  Every pair is computed (no pruning), and its value does not depend on what else is in the call.
 * Both calls replace md.rmsd(traj, frame) * 10 of evaluate/evaluators.py:656-662 applied once per candidate frame (with
 * dff_struct_rmsd: m launches, each reading all n queries again).
 *
 * Bytes of device workspace dff_rmsd_nearest needs (one 64-bit key per query of a pass of at most 2^20 queries: bounded
 * in n, independent of m); -1 on bad arguments. */
long long dff_rmsd_nearest_workspace_bytes(long long n, long long m, int n_beads);
/* rmsd_dev[s] = the smallest fp32-rounded RMSD of query s to a candidate, index_dev[s] (may be NULL) that candidate.
 * Tie rule: among candidates at the same fp32 RMSD the LOWEST index wins.  Non-finite rule: a query with a non-finite
 * coordinate gets NaN and -1; a candidate with a non-finite coordinate is never nearest; with no usable candidate
 * (m == 0, all candidates non-finite, or only the excluded one) the result is NaN and -1.
 * self_first >= 0 declares that query s IS candidate self_first + s: that pair is skipped (diversity, and chunked calls
 * within one ensemble); -1: no such pair.
 * Equal BIT FOR BIT to the row minimum and the first argmin of dff_rmsd_matrix (one per-pair routine serves both), and
 * bit-identical from call to call whatever the split of queries or candidates over workgroups and calls: the reduction is
 * an integer minimum over the keys (fp32 bits << 32 | index), no floating-point atomics.  m <= 2^31 - 1.
 * workspace_dev: >= dff_rmsd_nearest_workspace_bytes(n, m, n_beads) bytes, 8-byte aligned (DFF_EINVAL otherwise: the keys are
 * 64-bit words under an atomic minimum), contents irrelevant. */
int dff_rmsd_nearest(int device, const float* x_dev, long long n, const float* y_dev, long long m, int n_beads,
                     long long self_first, float* rmsd_dev, long long* index_dev, void* workspace_dev,
                     size_t workspace_bytes, void* stream);
/* The dense block for small problems (clustering, tests): out_dev[s * m + r] = RMSD of query s to candidate r, NaN where
 * either frame has a non-finite coordinate.  n * m <= 2^28 (DFF_EINVAL beyond). */
int dff_rmsd_matrix(int device, const float* x_dev, long long n, const float* y_dev, long long m, int n_beads,
                    float* out_dev, void* stream);

/* ---- superposition on a reference: rotations, aligned frames, mean-structure and RMSF sums (csrc/dff_superpose.hip) ----
 * The rotation that every RMSD call above solves for and discards.  Stateless like dff_struct_*: x_dev (n, n_beads, 3)
 * and ref_dev (n_beads, 3) fp32 in Angstrom on the device, 4 <= n_beads <= 64, frames independent; enqueued on `stream`
 * only, no synchronisation on the launch path; bad arguments are refused on the host before any device call.
 * R of a frame is the PROPER rotation (det R = +1: a mirror image is not matched) that minimises
 * sum_b |R a_b - r_b|^2, a_b = x_b - c_x and r_b = ref_b - c_ref the beads relative to the unweighted centroids; fp64
 * throughout: Horn's 4 x 4 key matrix as in dff_struct_rmsd, cyclic Jacobi with accumulated eigenvectors, R from the
 * formula quadratic in the unit quaternion (a half turn, q0 = 0, is an ordinary input).
 * Replaces traj.superpose(traj, 0), datasets/dataset_utils_empty.py:319-321 (ref_dev = frame 0).
 *
 * Bytes of device workspace dff_superpose needs for n frames when it accumulates statistics (one slice of 4 N + 1 doubles
 * per workgroup, at most 4096 workgroups: bounded in n); -1 on bad arguments. */
long long dff_superpose_workspace_bytes(long long n, int n_beads);
/* Every output may be NULL.
 *   aligned_dev (n, N, 3) fp32   R a_b + c_ref, rounded to fp32 once: frames land ON THE REFERENCE'S CENTROID, as mdtraj's
 *                                superpose leaves them.  In place: aligned_dev == x_dev (exactly the same pointer) is
 *                                supported -- a tile of 64 frames is read completely before any of it is written, and
 *                                tiles are disjoint; a PARTIAL overlap of the two arrays is undefined.
 *   rot_dev (n, 9) fp64          R, row-major.
 *   rmsd_dev (n) fp32            the quantity dff_struct_rmsd returns.
 *   dsum_dev (N, 3) fp64, dsq_dev (N) fp64, count_dev (1) uint64 -- OVERWRITTEN by the call, over the finite frames, with
 *                                d_b = (R a_b + c_ref) - ref_b in fp64, BEFORE the fp32 rounding of aligned_dev:
 *                                dsum = sum d_b, dsq = sum |d_b|^2, count = the number of finite frames.
 *                                mean structure = ref + dsum / count; RMSF_b^2 = dsq_b / count - |dsum_b / count|^2.
 * Non-finite rule: a frame with any non-finite coordinate gets NaN in all its aligned / rot / rmsd entries and takes part
 * in no sum; a reference with a non-finite coordinate makes every frame such a frame (count = 0).  Nothing is read back.
 * Degenerate rule: a frame whose key matrix is zero (all beads coincident: R = I) or whose largest eigenvalue is
 * degenerate (collinear frame or reference) gets A maximiser: finite, a proper rotation, reaching the minimal RMSD -- but
 * one of a continuum, not comparable entry by entry with another solver's.
 * n == 0 is a valid no-op that zeroes dsum / dsq / count.  With the three statistics NULL no workspace is needed;
 * otherwise workspace_dev: >= dff_superpose_workspace_bytes(n, n_beads) bytes, 8-byte aligned, contents irrelevant.
 * Deterministic: per-workgroup partials in the workspace, added in a fixed order by a second stage, no floating-point
 * atomics -- bit-identical from call to call with the same arguments (the rule of dff_kmeans_step). */
int dff_superpose(int device, const float* x_dev, long long n, int n_beads, const float* ref_dev,
                  float* aligned_dev, double* rot_dev, float* rmsd_dev,
                  double* dsum_dev, double* dsq_dev, uint64_t* count_dev,
                  void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- clustering one ensemble under the RMSD with a cutoff: neighbour bit-matrix and the greedy loop of Daura et al.,
 * `gmx cluster -method gromos` (csrc/dff_cluster.hip) ----
 * Stateless like the calls above; enqueued on `stream` only, no read-back and no synchronisation on the launch path, no
 * floating-point atomics; bad arguments are refused on the host before any device call; n == 0 is a valid no-op.
 * n <= 2^18 frames (8 GiB of bits; DFF_EINVAL beyond).
 *
 * The neighbour matrix of x_dev (n, n_beads, 3), fp32 in Angstrom, 4 <= n_beads <= 64, against itself, one BIT per pair:
 * adj_dev is n rows of W = ceil(n / 64) uint64_t words, every word overwritten.  Bit r & 63 of word s * W + (r >> 6) is
 * set when s != r, both frames are finite and d(s, r) <= cutoff as fp32, where d(s, r) is the value dff_rmsd_matrix(x, x)
 * writes at [min(s, r), max(s, r)], BIT FOR BIT (the same per-pair routine, the lower index as the query; each pair is
 * computed once).  The matrix is therefore symmetric by construction.  The diagonal bit is set for every finite frame by
 * definition; a frame with a non-finite coordinate has an all-zero row and column; bits at positions >= n are zero.
 * degree_dev (n) int32, may be NULL: the popcount of row s, self included.
 * cutoff: finite and >= 0.  The same matrix from call to call: integer ORs only. */
int dff_rmsd_neighbors(int device, const float* x_dev, long long n, int n_beads, float cutoff, uint64_t* adj_dev,
                       int* degree_dev, void* stream);
/* Bytes of device workspace dff_gromos_steps needs for n frames (the alive mask and one key); -1 on bad arguments. */
long long dff_gromos_workspace_bytes(long long n);
/* The greedy loop on a bit-matrix adj_dev as dff_rmsd_neighbors writes it (symmetric, the diagonal bit = "this frame takes
 * part"); one call enqueues n_steps >= 0 iterations.  restart != 0 first initialises the state: labels = -1, centers = -1,
 * sizes = 0, alive = the diagonal bits, progress_dev = {0 clusters, number of frames with a diagonal bit}.  The state
 * between calls is labels / centers / sizes / progress and the workspace: keep them untouched and pass restart = 0 to go on.
 * One iteration: among the alive frames the one with the largest popcount(row & alive), the LOWEST index among ties,
 * becomes the centre of cluster c = progress[0]; its alive neighbours, itself included, get label c; centers[c] = its
 * index, sizes[c] = their number; they leave alive; progress = {c + 1, unassigned - sizes[c]}.
 * When the largest alive degree is 1, every alive frame becomes a singleton cluster in ascending index order within that
 * same iteration -- the numbering the plain loop would give, without one iteration per singleton.  Clusters are capped
 * at max_clusters >= 1: frames beyond the cap keep -1.  Iterations after the end (progress[1] == 0) or after the cap are
 * no-ops decided on the device.  Clusters are numbered in order of creation: sizes are non-increasing.
 *   labels_dev (n) int32; centers_dev, sizes_dev int32, the first min(max_clusters, n) entries are used;
 *   progress_dev (2) int32; workspace_dev: >= dff_gromos_workspace_bytes(n) bytes, 8-byte aligned.
 * Integer arithmetic only: bit-identical from call to call and for every split of the iterations over calls.  No
 * workgroup waits on another: the phases of an iteration are separate launches. */
int dff_gromos_steps(int device, const uint64_t* adj_dev, long long n, int restart, int n_steps, int max_clusters,
                     int* labels_dev, int* centers_dev, int* sizes_dev, int* progress_dev, void* workspace_dev,
                     size_t workspace_bytes, void* stream);

/* ---- folding kinetics from an order parameter: native contacts per frame, core states along trajectories, runs of equal
 * labels (csrc/dff_kinetics.hip) ----
 * The reference looks at per-trajectory RMSD and contact dynamics (RmsdEvaluator.eval(save_dynamics=True),
 * _plot_rmsd_dynamics, _eval_bce_dynamics; evaluate/evaluators.py) and stops at plots; these calls turn such a series into
 * states, dwell runs and rates (the reductions over the runs stay on the host: evaluate.py, dwell_summary).
 * Stateless like the calls above: device pointers, enqueued on `stream` only, no read-back and no synchronisation on the
 * launch path; bad arguments are refused on the host before any device call; n == 0 is a valid no-op; bit-identical from
 * call to call; no floating-point atomics; no workgroup waits on another (the phases of a scan are separate launches).
 * Trajectories are passed as dff_transition_counts takes them: n_traj trajectories back to back, lengths_host[i] frames
 * each (sum = n), any n_traj; an empty trajectory holds no frame.
 *
 * The soft fraction of native contacts of Best, Hummer & Eaton (2013):
 *   q_dev[s] = (1 / P) sum_p 1 / (1 + exp(beta (r_p(s) - lambda r0_p))),   r_p(s) = |x_i - x_j| of pair p = (i_p, j_p) in frame s.
 * pairs_dev (P, 2) int32 and r0_dev (P) fp32 (Angstrom) on the device, P = n_pairs.  Everything in fp64 from the fp32
 * coordinates, the sum over the pairs in list order, rounded to fp32 once: a frame's value does not depend on what else is
 * in the call, or on how frames are split over workgroups or calls.  4 <= n_beads <= 64, 1 <= n_pairs <= N (N - 1) / 2,
 * beta and lambda finite and > 0.
 * A frame with a non-finite coordinate gets NaN.  The pair list is not read back: an index outside 0 .. N - 1, or i == j, is
 * detected on the device and EVERY frame then gets NaN; nothing is ever read out of bounds.  Huge finite coordinates give
 * 0, not NaN (exp overflows to +inf, 1 / (1 + inf) = 0). */
int dff_struct_native_q(int device, const float* x_dev, long long n, int n_beads, const int32_t* pairs_dev,
                        const float* r0_dev, int n_pairs, double beta, double lambda, float* q_dev, void* stream);
/* Bytes of device workspace dff_core_states and dff_label_runs need for n frames (one 16-byte carry per 2048 frames); -1
 * on bad arguments. */
long long dff_kinetics_workspace_bytes(long long n);
/* Dual-cutoff (core-set, "transition-based") state of every frame of the series cv_dev (n) fp32.  Per trajectory, in frame
 * order, with state = -1 at the trajectory's first frame:
 *   cv non-finite (NaN, +-inf)  -> state = -1: the history is reset, and the frame's label is -1;
 *   cv <= lo -> state = 0;   cv >= hi -> state = 1 (equality counts as inside the core);   otherwise the state is unchanged;
 *   labels_dev[t] = state.
 * A frame belongs to the last core it visited, so recrossings of a single threshold are no transitions; nothing leaks
 * across a trajectory boundary.  core_dev (n) int8, may be NULL: 0 / 1 for a frame inside a core, -1 otherwise.
 * lo < hi, both finite.  An inclusive maximum scan over integer keys (block scan, carry scan, apply: three launches per
 * group of up to 64 unequal, or any number of equal-length, trajectories): exact.
 * workspace_dev: >= dff_kinetics_workspace_bytes(n) bytes, 8-byte aligned, contents irrelevant. */
int dff_core_states(int device, const float* cv_dev, long long n, const long long* lengths_host, int n_traj,
                    float lo, float hi, int32_t* labels_dev, int8_t* core_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);
/* Run-length encoding of labels_dev (n) int32 inside trajectories: a run is a maximal stretch of consecutive frames of ONE
 * trajectory with the same label (any int32, -1 included).  Runs come out in ascending run_start:
 *   run_start_dev[r] its first frame, run_length_dev[r] its frames, run_label_dev[r] its label,
 *   run_flags_dev[r] bit 0: the run begins at its trajectory's first frame, bit 1: it ends at its trajectory's last frame.
 * n_runs_dev (1) receives the TRUE number of runs; only the first max_runs >= 0 are written, entries beyond are not
 * touched (the run arrays may be NULL when max_runs == 0).  n == 0 writes n_runs = 0 (when n_runs_dev is given).
 * The scan of dff_core_states with a sum next to the maximum: exact.  Also the lifetimes of the states that
 * dff_struct_tic_assign labels.  workspace_dev: as for dff_core_states. */
int dff_label_runs(int device, const int32_t* labels_dev, long long n, const long long* lengths_host, int n_traj,
                   long long max_runs, long long* run_start_dev, long long* run_length_dev, int32_t* run_label_dev,
                   uint8_t* run_flags_dev, long long* n_runs_dev,
                   void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- transition paths: the previous AND the next core of every frame, frame classes, the table of paths
 * (csrc/dff_paths.hip; evaluate.py: path_states, transition_paths, path_histograms, tp_probability, empirical_committor,
 * TransitionPathEvaluator) ----
 * Stateless like the calls above: device pointers, enqueued on `stream` only, no read-back and no synchronisation on the
 * launch path; bad arguments are refused on the host before any device call; bit-identical from call to call and independent
 * of the workspace's prior contents; integers only, no atomics; no workgroup waits on another.  cv_dev, lengths_host, lo and
 * hi are those of dff_core_states.
 * Bytes of device workspace dff_path_states needs for n frames (one 32-byte carry per 2048 frames); -1 on bad arguments. */
long long dff_path_states_workspace_bytes(long long n);
/* The code of frame t: non-finite; A (cv <= lo); B (cv >= hi, equality inside); between.  Per trajectory:
 *   prev_dev[t] / t_prev_dev[t]   walk back from t (inclusive) to the first frame that is not between: A -> 0, B -> 1, with its
 *       frame index in the concatenated series; a non-finite frame, or the trajectory's start reached -> -1 / -1.  prev is,
 *       bit for bit, what dff_core_states writes to labels_dev (as int8).
 *   next_dev[t] / t_next_dev[t]   the mirror image: walk forward (inclusive) to the trajectory's end.
 *   class_dev[t]   0 / 1 in core A / B; for a frame between the cores with prev >= 0 and next >= 0: 2 on a path A -> B,
 *       3 on a path B -> A, 4 on a loop out of A and back, 5 on a loop out of B and back; -1 otherwise (non-finite, or the
 *       history unknown on either side).
 * Each of the five (n) arrays may be NULL.  Nothing crosses a trajectory boundary or a non-finite frame, in either direction.
 * The path table: one record per frame e that is in a core, is not its trajectory's first frame, and has prev[e - 1] >= 0 and
 * != the core of e:  path_exit_dev[r] = t_prev[e - 1], path_entry_dev[r] = e, path_dir_dev[r] = the core of e (1: A -> B), in
 * ascending entry.  entry - exit >= 1 frames is the path's duration (1: a direct jump).  n_paths_dev (1) receives the TRUE
 * number of paths; only the first max_paths >= 0 records are written, entries beyond are not touched (the arrays may be NULL
 * when max_paths == 0).  n_paths_dev == NULL: no table.  n == 0 writes n_paths = 0 (when n_paths_dev is given).
 * One scan in both directions (block scan, carry scan, apply: three launches per group of up to 64 unequal, or any number of
 * equal-length, trajectories): exact.
 * workspace_dev: >= dff_path_states_workspace_bytes(n) bytes, 8-byte aligned, contents irrelevant. */
int dff_path_states(int device, const float* cv_dev, long long n, const long long* lengths_host, int n_traj,
                    float lo, float hi,
                    int8_t* prev_dev, int8_t* next_dev, long long* t_prev_dev, long long* t_next_dev, int8_t* class_dev,
                    long long max_paths, long long* path_exit_dev, long long* path_entry_dev, int8_t* path_dir_dev,
                    long long* n_paths_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- lagged products inside trajectories: the sums behind the autocorrelation function of an observable, its integrated
 * autocorrelation time and the effective sample size (csrc/dff_autocorr.hip) ----
 * The reference reports point estimates from its trajectories and no uncertainty; these sums give the relaxation time of a
 * scalar or few-component observable (Q, the RMSD to the folded structure, the leading TICs) without a state definition,
 * and n_eff = n / (2 tau_int) for the error bar of every mean (evaluate.py: autocorrelation, RelaxationEvaluator).
 * Stateless like the calls above: device pointers, enqueued on `stream` only, no read-back and no synchronisation on the
 * launch path; bad arguments are refused on the host before any device call; bit-identical from call to call and
 * independent of the workspace's prior contents; no floating-point atomics -- per-workgroup partials in the workspace are
 * added in a fixed order by a second stage; no workgroup waits on another.
 * Trajectories are passed as dff_transition_counts takes them: n_traj trajectories back to back, lengths_host[i] frames
 * each (sum = n), any n_traj; an empty trajectory holds no frame.
 *
 * series_dev (n, d) fp64 row-major, 1 <= d <= 8; 0 <= max_lag <= 65535; shift_dev (d) fp64, finite, NULL = 0.
 *   g_t = series[t] - shift, in fp64.  A frame is USABLE when all its d components are finite.
 *   P_l = { t : t and t + l lie in the same trajectory and both frames are usable },   l = 0 .. max_lag.
 * The call overwrites, each sum over t in P_l and in fp64:
 *   count_dev[l] = |P_l|          sx_dev[l, c] = sum g_{t,c}          sy_dev[l, c] = sum g_{t+l,c}
 *   sxy_dev[l, c] = sum g_{t,c} g_{t+l,c}
 * sxy_dev, sx_dev, sy_dev are (max_lag + 1, d) fp64, count_dev (max_lag + 1) uint64; a lag that no trajectory reaches gets
 * zeros.  sx_dev, sy_dev and count_dev may each be NULL (with all three NULL only the products are formed); sxy_dev may
 * not.  n == 0 is a valid no-op that zeroes the outputs.  Cross-correlations between components are not computed.
 * Work: sum_l |P_l| <= n (max_lag + 1) pairs, four fp64 FMAs per pair and component (one without sx, sy and count).
 * workspace_dev: >= the bytes the workspace call below gives, 8-byte aligned, contents irrelevant: 4 n bytes (the frames
 * left in each frame's trajectory) plus the partials, which do not grow with n (at most ~2048 workgroups' worth: under 64 MB
 * for any d and max_lag; 30 MB at n = 10^6, d = 2, max_lag = 4096). */
/* Bytes of device workspace the call below needs (0 at n == 0); -1 on bad arguments. */
long long dff_autocorr_workspace_bytes(long long n, int d, int max_lag);
int dff_autocorr(int device, const double* series_dev, long long n, int d, const long long* lengths_host, int n_traj,
                 int max_lag, const double* shift_dev, double* sxy_dev, double* sx_dev, double* sy_dev,
                 uint64_t* count_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Markov state models at microstate resolution: k-means and transition counts for up to DFF_MSM_MAXK states, and the
 * sweeps of the reversible maximum-likelihood estimator (csrc/dff_msm.hip) ----
 * What follows the four preset states of the reference's notebook: a few hundred k-means microstates in TIC space, count
 * matrices at several lag times, a reversible transition matrix with its stationary distribution, implied timescales
 * against the lag (evaluate.py: MicrostateKMeans, MarkovStateModel, implied_timescales, MsmEvaluator).  The K <= 64 calls
 * above keep their limit and their kernels; these are their counterparts for many states.
 * Stateless like the calls above: device pointers, enqueued on `stream` only, no read-back and no synchronisation on the
 * launch path; n == 0 is a valid no-op that still zeroes or overwrites what the call zeroes or overwrites; bad arguments
 * are refused on the host before any device call; no floating-point atomics; no workgroup waits on another; bit-identical
 * from call to call, independent of the workspace's prior contents and of every debug knob. */
#define DFF_MSM_MAXK 1024
/* Points per workgroup of the call below: a compile-time constant.  With (n, d, K) it fixes the order of every sum. */
int dff_micro_chunk(void);
/* Bytes of device workspace the call below needs for n points when it accumulates: ceil(n / chunk) rows of
 * K (d + 1) + 1 doubles (56 MB of 2^20 bytes at n = 819 200, d = 8, K = 1024); -1 on bad arguments. */
long long dff_micro_kmeans_workspace_bytes(long long n, int d, int K);
/* One Lloyd iteration with many centres: the arguments, the outputs and the assignment rule (fp64, one FMA per
 * coordinate in order, centres in index order, strict <, a non-finite point -> label -1, d2 = NaN, in no accumulator) are
 * those of dff_kmeans_step, so for K <= 64 labels_dev and dist2_dev are bit-identical to its.  1 <= d <= 8,
 * 1 <= K <= DFF_MSM_MAXK.  Every output may be NULL; with the three accumulators NULL the call only assigns and needs no
 * workspace.  sums_dev, counts_dev and inertia_dev are OVERWRITTEN.  One workgroup per chunk of points, the centres in
 * LDS; a chunk's members are added per accumulator in point order, the chunks' partials in chunk order by a second
 * stage: the order of summation depends on (n, d, K) and the chunk size alone (sums and inertia are therefore NOT
 * bit-identical to dff_kmeans_step's, which sums in another order).  workspace_dev 8-byte aligned. */
int dff_micro_kmeans_step(int device, const double* pts_dev, long long n, int d, const double* centers_dev, int K,
                          int32_t* labels_dev, double* dist2_dev, double* sums_dev, uint64_t* counts_dev,
                          double* inertia_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Sliding-window transition counts between many states: arguments and semantics of dff_transition_counts with
 * 1 <= K <= DFF_MSM_MAXK, 1 <= n_lags <= 8; counts_dev (n_lags, K, K) is zeroed by the call.  For K > 64: 64-bit integer
 * atomics on global memory, equal (lag, i, j) aggregated inside a wave first.  For K <= 64 the call launches the
 * LDS-privatised kernel of dff_transition_counts itself (measured faster there: a metastable path hammers a few diagonal
 * counters), so its result is that call's.  Integer counting either way: exact, the same from call to call. */
int dff_micro_transition_counts(int device, const int32_t* labels_dev, long long n, const long long* lengths_host,
                                int n_traj, const int32_t* lags_host, int n_lags, int K, uint64_t* counts_dev, void* stream);
/* Bytes of device workspace the call below needs (two vectors of K doubles); -1 on bad arguments. */
long long dff_msm_workspace_bytes(int K);
/* n_steps sweeps of the fixed-point iteration of the reversible maximum-likelihood transition matrix (Bowman et al. 2009;
 * Prinz et al. 2011, algorithm 1 in its plain form) on a strongly connected set of K states:
 *   q_j = c_j / x_j,     x_i' = sum_j S_ij / (q_i + q_j),
 * sym_dev (K, K) fp64 row-major = S = C + C^T, rowc_dev (K) = c_i = sum_j C_ij > 0, x_dev (K) in/out, x_i > 0 (the host
 * starts from x_i = sum_j S_ij / 2).  A pair with S_ij == 0 adds exactly +0.0 whatever its quotient would be (the quotient is
 * formed and discarded by a select, also where q_j is NaN).  x is not renormalised: the map is homogeneous of degree 1.
 * T_ij = S_ij / (q_i + q_j) / x_i and pi = x / sum x are left to the
 * caller.  Every row sum is taken in one order (64 lanes stride over j, then a butterfly over the wave).
 * err_dev (n_steps), may be NULL: err_s = max_i |x_i' - x_i| / x_i of sweep s.
 * A row with c_i <= 0 or x_i <= 0 (or either NaN) gets x_i = NaN, from the next sweep on so does every row j with
 * S_ij != 0, and err_s is NaN from that sweep on; nothing is read back to check it.
 * All n_steps sweeps are enqueued without a host read; n_steps == 0 leaves x_dev alone.  1 <= K <= DFF_MSM_MAXK,
 * n_steps >= 0, workspace_dev 8-byte aligned, contents irrelevant. */
int dff_msm_reversible_steps(int device, const double* sym_dev, const double* rowc_dev, int K, double* x_dev, int n_steps,
                             double* err_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* For benchmarks, process-wide: which kernel runs the sweeps.  0 = by K (the default), 1 = one launch per sweep,
 * 2 = one workgroup that loops over all sweeps (per problem in dff_msm_reversible_steps_batched, which the knob forces
 * too).  The results are the same bits either way. */
int dff_debug_msm_driver(int driver);
/* Host only: the driver a call with K states would take now, 1 or 2 as above; -1 on a bad K. */
int dff_msm_driver_for(int K);

/* ---- Bootstrap error bars for the models above: the count matrices of B weighted resamples in one pass over the labels,
 * and the estimator's sweeps on B problems per launch (csrc/dff_msm_batch.hip; evaluate.py: bootstrap_msm) ----
 * The conventions of the block above hold: device pointers, `stream` only, no read-back, no synchronisation, refusals on the
 * host before any device call, no floating-point atomics, no workgroup waits on another, bit-identical from call to call
 * and independent of the workspace's prior contents.  Host tables reach the device as kernel arguments. */
/* Bytes of device workspace the call below needs (the trajectory and unit start tables); -1 on bad arguments. */
long long dff_micro_resampled_counts_workspace_bytes(int n_traj, int n_units);
/* counts_dev[b][i][j] = sum of weights_dev[b][unit(t)] over every frame t with labels[t] = i, labels[t + lag] = j, t and
 * t + lag in the same trajectory and both labels in 0 .. K - 1.  labels_dev, n, lengths_host, n_traj as
 * dff_micro_transition_counts; unit_lengths_host (n_units) are the resampling units, back to back, summing to n (they
 * partition the FRAMES and need not coincide with trajectories: a pair belongs to the unit of its first frame, so no pair
 * is lost and with all weights 1 every slice is dff_micro_transition_counts' matrix); weights_dev (B, n_units) uint32 is
 * the multiplicity of unit u in resample b; counts_dev (B, K, K) is zeroed by the call (also at n == 0).
 * 1 <= K <= DFF_MSM_MAXK, 1 <= B <= 4096, B K^2 <= 2^28, 1 <= n_units <= 2^20, n <= 2^31 (no 64-bit sum can overflow),
 * lag >= 1.  64-bit integer atomics on global memory, equal (i, j, unit) aggregated inside a wave first, one atomic per
 * aggregate and resample with a non-zero weight: exact, the same from call to call.  workspace_dev 8-byte aligned. */
int dff_micro_resampled_counts(int device, const int32_t* labels_dev, long long n, const long long* lengths_host, int n_traj,
                               const long long* unit_lengths_host, int n_units, int lag, int K, const uint32_t* weights_dev,
                               int B, uint64_t* counts_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Bytes of device workspace the call below needs (two vectors of B Kmax doubles and B descriptors); -1 on bad arguments. */
long long dff_msm_batched_workspace_bytes(int B, int Kmax);
/* dff_msm_reversible_steps on B problems at once.  Problem b has 1 <= K_b = ks_host[b] <= Kmax <= DFF_MSM_MAXK states, its S
 * a COMPACT (K_b, K_b) row-major matrix at sym_dev + b Kmax^2, its c at rowc_dev + b Kmax and its x at x_dev + b Kmax; what
 * lies beyond K_b in a slot is never read or written.  For every problem that is not skipped, x and err_dev[:, b] after the
 * call are bit-identical to dff_msm_reversible_steps(sym_b, rowc_b, K_b, x_b, n_steps, err_b): the same order of every row
 * sum, the same select for S_ij == 0, the same NaN rules, confined to the problem they arise in.  skip_host (B, may be
 * NULL): a problem with a non-zero byte keeps its x and gets err_dev[:, b] = 0.  err_dev (n_steps, B), may be NULL.
 * One launch per sweep covers the rows of all live problems, or one looping workgroup per live problem runs all sweeps:
 * the latter where dff_msm_reversible_steps would loop for the largest live problem, and wherever there are enough live
 * problems for it (measured: dff_msm_batched_driver_for).  dff_debug_msm_driver forces either; both give the same bits.  1 <= B <= 4096, n_steps >= 0 (0 leaves everything alone), workspace_dev 8-byte
 * aligned, contents irrelevant. */
int dff_msm_reversible_steps_batched(int device, const double* sym_dev, const double* rowc_dev, const int32_t* ks_host,
                                     const uint8_t* skip_host, int B, int Kmax, double* x_dev, int n_steps, double* err_dev,
                                     void* workspace_dev, size_t workspace_bytes, void* stream);
/* Host only: the driver a batched call with B live problems, the largest of Kmax states, would take now: 1 = one launch per
 * sweep, 2 = one looping workgroup per problem; -1 on bad arguments. */
int dff_msm_batched_driver_for(int B, int Kmax);

/* ---- Mean first-passage times and committors of the reversible models above: the Dirichlet problem on a flux matrix, P
 * problems per call, one workgroup per problem (csrc/dff_msm_passage.hip; evaluate.py: mfpt, committor, reactive_flux,
 * bootstrap_passage) ----
 * Problem p has K_p = ks_host[p] states, a symmetric non-negative flux matrix X (only its relative scale matters), a role per
 * state (0 = interior, 1 = boundary), boundary values g and a source s, and asks for u with
 *   u_i = g_i on the boundary,     sum_{j != i} X_ij (u_i - u_j) = (sum_j X_ij) s_i on every interior state,
 * which is (u - T u)_i = s_i for T_ij = X_ij / sum_j X_ij.  The mean first-passage time to a set: boundary = the set, g = 0,
 * s = the lag time.  The committor from A to B: boundary = A and B, g = 1 on B and 0 on A, s = 0.
 * flux_dev (n_flux, Kmax, Kmax) fp64: matrix m is a COMPACT (K, K) row-major matrix at flux_dev + m Kmax^2; problem p reads
 * matrix flux_of_host[p] (NULL: matrix p, n_flux >= P) as (K_p, K_p), so the problems that share a matrix have the same K_p.
 * role_dev int32, g_dev, s_dev, u_dev fp64: (P, Kmax), problem p in the first K_p entries of row p; g is read at boundary states
 * only, s at interior states only, u is written at 0 .. K_p - 1 only.  status_dev (P) int32:
 *    0      solved (also when every state is boundary: u = g)
 *   -1      no boundary state                                                    u = NaN over 0 .. K_p - 1
 *   -2      a role outside {0, 1} (it wins over -1)                              u = NaN
 *   1 + i   the pivot of state i (full index) was not a finite positive number   u = NaN
 * The interior indices are compacted in index order, W = diag(d) - offdiag(X_II) is formed with d_i = sum_{j != i} X_ij SUMMED
 * over the whole row (never as a difference of two nearly equal numbers; in ONE order: 64 partial sums, partial l over
 * j = l, l + 64, ..., then a butterfly -- on an ill-conditioned W another order of this sum moves the exact solution by more
 * than a good solver's error), b_i = (d_i + X_ii) s_i + sum_{j boundary} X_ij g_j, and W = L D L^T is factored without pivoting
 * and without square roots (the pivots are D's entries), followed by the two substitutions.  Besides the row sums only the lower
 * triangle of X_II is read: an asymmetric X is not detected as such.  The pivot of state i fails when it is not finite or not
 * above n 2^-52 d_i (n the interior count): an interior component that cannot reach the boundary is singular in exact arithmetic
 * and leaves a pivot of rounding size, zero or below, while the pivots of a connected problem stay above that guard up to
 * cond(W) ~ 1 / (n 2^-52).  It also fails when the state's row, X_ii included, or its b_i (g, s) holds a NaN or an infinity:
 * status 0 never comes with a NaN in u.  A failed problem touches no other.  After a solved problem of the blocked path the first
 * four doubles of its slice of the workspace hold, for benchmarks, the 100 MHz ticks spent in formation, panels, trailing updates
 * and back substitution.  Up to dff_msm_dirichlet_lds_limit interior states the triangle is factored in LDS; above, a blocked
 * right-looking factorisation (panels of 32 columns, 64 x 64 trailing tiles on the fp64 VALU) runs in the problem's slice of the
 * workspace.  The bits of a problem's u and status follow from its own inputs and from the path alone: not from P, its place in
 * the batch, its neighbours, the workspace's prior contents or the call; the two paths need not agree bit for bit.
 * 1 <= K_p <= Kmax <= DFF_MSM_MAXK, 1 <= P <= 16384, 1 <= n_flux <= 16384; device pointers, `stream` only, no read-back, refusals on
 * the host before any device call, no atomics, no workgroup waits on another.  workspace_dev 8-byte aligned, contents irrelevant. */
/* Bytes of device workspace the call below needs (P descriptors and P slices of Kmax (Kmax + 32) doubles); -1 on bad arguments. */
long long dff_msm_dirichlet_workspace_bytes(int P, int Kmax);
/* The largest interior count that is factored out of LDS (a compile-time constant). */
int dff_msm_dirichlet_lds_limit(void);
int dff_msm_dirichlet_solve(int device, const double* flux_dev, int n_flux, const int32_t* flux_of_host, const int32_t* ks_host,
                            int P, int Kmax, const int32_t* role_dev, const double* g_dev, const double* s_dev, double* u_dev,
                            int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* For tests and benchmarks, process-wide: 0 = the path follows the interior count (the default), 1 = every problem in LDS (a call
 * with a K_p above the limit + 1 is then refused), 2 = every problem on the blocked path; 3 and 4 = as 2, with the trailing update
 * on the fp64 VALU (3) or on v_mfma_f64_16x16x4_f64 (4) instead of the library's choice between them.  The two trailing updates
 * sum in different orders: each gives its own, reproducible bits. */
int dff_debug_msm_dirichlet_path(int path);

/* ---- The k algebraically largest eigenvalues, and optionally their eigenvectors, of P dense symmetric fp64 matrices of
 * differing sizes, one workgroup per problem (csrc/dff_sym_eig.hip; evaluate.py: msm_spectrum, MarkovStateModel.eigenvectors,
 * eigensolver="device") ----
 * Problem p is a COMPACT (K_p, K_p) row-major matrix at a_dev + p Kmax^2, K_p = ks_host[p] (the layout of
 * dff_msm_reversible_steps_batched); it is read-only, and only its lower triangle is read: an asymmetric matrix is not detected
 * as such.  w_dev (P, k): the kk = min(k, K_p) largest eigenvalues of problem p, descending, NaN from index K_p on.  v_dev
 * (P, k, Kmax), or NULL when no vectors are wanted: row j is the eigenvector of eigenvalue j, written at 0 .. K_p - 1 only (rows
 * j >= K_p are NaN there); unit 2-norm, the component of largest magnitude positive, the lowest index winning a tie.  The
 * eigenvalues of a call with vectors are bit-identical to those of a call without.  status_dev (P) int32:
 *   0   solved
 *   1   a non-finite entry in the lower triangle               every output of the problem is NaN
 *   2   a vector's inverse iteration did not reach its growth   the eigenvalues are valid, the problem's vectors NaN
 * Status 0 never comes with a NaN at an index below K_p; a failed problem touches no other.
 * Per problem: Householder reduction to tridiagonal form on a working copy (unblocked; a column that is already zero below the
 * sub-diagonal gets tau = 0 and no division, so diagonal and tridiagonal inputs are legal; column norms are taken of the column
 * divided by its largest entry), the eigenvalues by Sturm-count multisection with dstebz's pivmin safeguard until no shift
 * lies strictly inside a bracket, the vectors by inverse iteration as in dstein (tridiagonal LU with partial pivoting, at most
 * five solves, eigenvalues closer than 10 ulp perturbed apart, modified Gram-Schmidt against every earlier vector of the problem:
 * exactly repeated eigenvalues get an orthonormal basis), then the stored reflectors.  Up to dff_sym_eig_lds_limit states the
 * packed triangle lives in LDS; above, the same algorithm runs in the problem's slice of the workspace.  After the call the
 * first three doubles of a problem's slice hold, for benchmarks, the 100 MHz ticks spent in reduction, bisection and vectors.
 * The bits of a problem's outputs follow from its own inputs, k and the path alone: not from P, its place in the batch, its
 * neighbours, the workspace's prior contents or the call; the two paths need not agree bit for bit.
 * 1 <= K_p <= Kmax <= DFF_MSM_MAXK, 1 <= P <= 16384, 1 <= k <= 32; device pointers, `stream` only, no read-back, refusals on the
 * host before any device call, no atomics, no workgroup waits on another.  workspace_dev 8-byte aligned, contents irrelevant. */
/* Bytes of device workspace the call below needs (P state counts and P slices of 4 + Kmax^2 doubles); -1 on bad arguments. */
long long dff_sym_eig_workspace_bytes(int P, int Kmax);
/* The largest K_p that is reduced out of LDS (a compile-time constant). */
int dff_sym_eig_lds_limit(void);
int dff_sym_eig_topk(int device, const double* a_dev, const int32_t* ks_host, int P, int Kmax, int k, double* w_dev,
                     double* v_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* For tests and benchmarks, process-wide: 0 = the path follows K_p (the default), 1 = every problem in LDS (a call with a K_p
 * above the limit is then refused), 2 = every problem in the workspace. */
int dff_debug_sym_eig_path(int path);

/* ---- Row vectors through a transition matrix, step after step: w_{s+1} = w_s T for up to 16 start vectors per problem and, after
 * every step, their scalar products with up to 16 observables; P problems per call, one workgroup per problem for all S steps
 * (csrc/dff_msm_propagate.hip; evaluate.py: msm_propagate, msm_relaxation, msm_autocorrelation, chapman_kolmogorov) ----
 * Problem p has K_p = ks_host[p] states and reads matrix mat_of_host[p] (NULL: matrix p, n_mat >= P): a COMPACT (K_p, K_p) row-major
 * fp64 matrix at t_dev + m Kmax^2 (the layout of dff_sym_eig_topk).  Problems may share a matrix; those that do must agree on K_p.
 * The matrix is a GENERAL dense matrix: it need be neither stochastic nor reversible.  w0_dev (P, M, Kmax): M start row vectors;
 * obs_dev (P, R, Kmax): R observables; both read at indices below K_p only.  With w_0 = w0 and w_{s+1} = w_s T,
 *   out_dev (P, S + 1, M, R):   out[s][m][r] = sum_j w_s[m][j] obs[r][j],   s = 0 .. S
 *   w_last_dev (P, M, Kmax), or NULL: w_S at indices below K_p; elements from K_p on are not written.
 * status_dev (P) int32:
 *   0   solved
 *   1   a non-finite entry in the problem's matrix, start vectors or observables (below K_p)     every output of the problem is NaN
 *   2   finite inputs, but the chain overflowed and produced a NaN (inf - inf, 0 inf)             every output of the problem is NaN
 * Status 0 never comes with a NaN; a failed problem touches no other.
 * Arithmetic: (w T)[m][j] is ONE chain of fused multiply-adds over i = 0 .. K_p - 1, started from +0, on both paths; out[s][m][r]
 * is 32 such chains over j = c, c + 32, ..., added by a fixed tree.  The bits of out[.][m][.] and w_last[m] follow from the matrix,
 * row m of w0, obs and the path alone: not from P, the problem's place in the batch, its neighbours, the workspace, the call, the
 * other start rows or M (a problem with M = 3 equals three M = 1 problems that share its matrix, bit for bit; likewise R), nor
 * from S (the first S1 + 1 steps of a longer run are the run to S1).  Up to dff_msm_propagate_lds_limit states the matrix is
 * copied into LDS once and all steps run from there; above, it streams from global memory once per step (all M rows per pass).
 * The two paths run the same chains, so they agree bit for bit as well; that is not part of the contract.
 * 1 <= K_p <= Kmax <= DFF_MSM_MAXK, 1 <= P, n_mat <= 16384, 1 <= M, R <= 16, 0 <= S <= 65535, P (S + 1) M R <= 2^28; device pointers,
 * `stream` only, no read-back, refusals on the host before any device call, no atomics, no workgroup waits on another.
 * workspace_dev 8-byte aligned, contents irrelevant. */
/* Bytes of device workspace the call below needs (P problem descriptors); -1 on bad arguments. */
long long dff_msm_propagate_workspace_bytes(int P, int Kmax, int M, int R);
/* The largest K_p that is propagated out of LDS (a compile-time constant). */
int dff_msm_propagate_lds_limit(void);
int dff_msm_propagate(int device, const double* t_dev, int n_mat, const int32_t* mat_of_host, const int32_t* ks_host, int P,
                      int Kmax, const double* w0_dev, int M, const double* obs_dev, int R, int S, double* out_dev,
                      double* w_last_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* For tests and benchmarks, process-wide: 0 = the path follows K_p (the default), 1 = every problem in LDS (a call with a K_p
 * above the limit is then refused), 2 = every problem with its matrix streamed from global memory. */
int dff_debug_msm_propagate_path(int path);

/* ---- What dff_msm_dirichlet_solve, dff_sym_eig_topk and dff_msm_propagate launch: at most two kernels, each one workgroup per
 * problem, each taking the problems whose size lies in lo .. hi and leaving the others to the other launch.  A problem's size is
 * K_p; for the Dirichlet solver it is the interior count, at most K_p - 1. */
typedef struct {
    int32_t launched;       /* 0: this launch does not happen, the other fields are 0 */
    int32_t path;           /* 1 = LDS, 2 = the workspace / global memory */
    int32_t lo, hi;         /* own_lo, own_hi as the kernel is handed them */
    int32_t sized_for;      /* the size its dynamic LDS is computed for */
    int32_t lds_bytes;
} dff_msm_batch_launch;
typedef struct {
    dff_msm_batch_launch launch[2];   /* the LDS kernel's, then the other path's */
} dff_msm_batch_plan;
/* Host only, for tests, no GPU needed: the plan of `call` ("dirichlet", "eig" or "propagate") for P problems of ks_host[p] states
 * under that call's debug path as it stands -- the function the call itself goes through.  It refuses what the call refuses about
 * P, Kmax, ks_host and a forced LDS path, in the call's words. */
int dff_debug_msm_batch_plan(const char* call, const int32_t* ks_host, int P, int Kmax, dff_msm_batch_plan* out);

/* ---- Hidden Markov models: one E-step of Baum-Welch over all chains of a set of labelled trajectories, by a chunked
 * forward-backward (csrc/dff_hmm.hip; evaluate.py: hmm_estep_solver, HiddenMarkovModel, HmmEvaluator) ----
 * The model: m hidden states, 1 <= m <= DFF_HMM_MAXM, K observed symbols, 1 <= K <= DFF_MSM_MAXK; fp64 on the device: trans_dev
 * (m, m) = A, emit_dev (m, K) = B, init_dev (m) = p0.  Their rows need not be normalised, and the call does not normalise them.
 * The observations are the int32 labels of every MSM call (labels_dev (n), trajectories of lengths_host back to back).  At lag
 * tau, trajectory r with offset f = 0 .. tau - 1 is one CHAIN: the frames f, f + tau, f + 2 tau, ... of r.  Chains are ordered
 * r-major, f-minor (chain r tau + f); a chain without a frame contributes nothing (its chain_loglik is 0); every frame belongs to
 * exactly one chain.  A NEGATIVE label is a missing observation: its emission factor is 1 for every hidden state, and it adds
 * nothing to the emission counts.
 * With M_t = A diag(B[:, o_t]): alpha_t ~ alpha_{t-1} M_t (alpha_0 = p0 B[:, o_0]), beta_{t-1} ~ M_t beta_t.  A chain is cut into chunks of
 * dff_hmm_chunk() of its own frames.  (1) Per chunk P = prod M_t over its frames (the chain's first frame left out), row by row;
 * after every step a row is rescaled by the power of two of its own sum -- exactly -- and the exponents are added up.  (2) Per
 * chain, serially over its chunks: the alpha entering and the beta leaving every chunk (alpha <- alpha P, beta <- P beta, rescaled by powers
 * of two), and the chain's log-likelihood ln(sum alpha_last) + ln 2 * (the exponents).  (3) Per chunk the forward recursion again
 * from the true alpha and the backward one from the true beta; per frame the posterior gamma_t = alpha_t beta_t, normalised by its own sum,
 * and the pair posterior xi_t(i, j) ~ alpha_{t-1}(i) A_ij B_j(o_t) beta_t(j), normalised by its own sum and added up per chunk in the
 * backward pass's order.  (4) stats_dev, packed: loglik (1) | xi (m, m) | gamma0 (m) | gamma_sym (m, K) --
 *   loglik      the chains' log-likelihoods, added in chain order
 *   xi          the chunks' sums of xi_t, added in chunk order
 *   gamma0      gamma of the chains' first frames, added in chain order
 *   gamma_sym   Gamma[i, s] = sum of gamma_t(i) over the frames with o_t = s: groups of 1024 frames, every accumulator owned by one thread
 *               and added in frame order, the groups added in order.
 * chain_loglik_dev (n_traj lag), or NULL; post_dev (n, m): the posteriors in frame order, or NULL (then they live in the
 * workspace).  status_dev: ONE int32 --
 *   0   success
 *   1   a parameter entry is non-finite or negative
 *   3   a label >= K
 *   2   some chain has likelihood zero under the model (its forward vector vanished, or overflowed)
 * in that order of precedence; on any non-zero status every output is NaN.  Status 0 never comes with a NaN.
 * What the bits depend on: a chain's chain_loglik and its frames' posteriors follow from that chain's labels, the parameters and
 * the chunk length alone -- not from the other chains, the chain's place among them, the lag or trajectory it was cut from, or the
 * workspace; stats is in addition a function of the order of the chains and of the frames.  Everything is identical from call
 * to call, and stats is the same with post_dev given or NULL.
 * lag >= 1, n_traj lag <= 2^20 chains, n <= 2^31; device pointers, `stream` only, no read-back, refusals on the host before any
 * device call, no floating-point atomics, no workgroup waits on another.  workspace_dev 8-byte aligned, contents irrelevant. */
#define DFF_HMM_MAXM 8
/* The chunk length (a compile-time constant). */
int dff_hmm_chunk(void);
/* Host only: the chains (n_traj lag, empty ones included) and chunks of a call; either output may be NULL. */
int dff_hmm_plan(const long long* lengths_host, int n_traj, int lag, long long* n_chains, long long* n_chunks);
/* Bytes of device workspace the call below needs (the trajectory table, the parameters, per chunk the product and the two
 * carries, per chain a log-likelihood, the (n, m) posteriors and per 1024 frames K m emission counts); -1 on bad arguments. */
long long dff_hmm_workspace_bytes(long long n, const long long* lengths_host, int n_traj, int lag, int m, int K);
int dff_hmm_estep(int device, const int32_t* labels_dev, long long n, const long long* lengths_host, int n_traj, int lag,
                  const double* trans_dev, const double* emit_dev, const double* init_dev, int m, int K, double* stats_dev,
                  double* chain_loglik_dev, double* post_dev, int32_t* status_dev, void* workspace_dev, size_t workspace_bytes,
                  void* stream);
/* For benchmarks, process-wide: 0 = the whole call (the default); 1 .. 5 = the call stops after its parameter launch, the chunk
 * products, the carries, the apply pass, the emission counts -- the share of every launch, by differences.  The outputs of a
 * call that stopped early are unfinished. */
int dff_debug_hmm_stages(int stages);

/* ---- Hidden Markov models: Baum-Welch on the device, n_steps iterations per call (csrc/dff_hmm_mstep.hip; evaluate.py:
 * hmm_fit_solver, HiddenMarkovModel(m_step="device"), bootstrap_hmm) ----
 * Limits, refusals (on the host, before any device call), chains, chunks and missing observations are those of dff_hmm_estep;
 * additionally n_steps >= 1, accuracy > 0, rev_tol > 0, rev_max_sweeps >= 1, reversible 0 or 1, and dff_debug_hmm_stages must be 0.
 * The call only enqueues on `stream`: no read-back, no floating-point atomics, no workgroup waits on another; the trajectory
 * table is uploaded once per call.  trans_dev (m, m), emit_dev (m, K), init_dev (m) are read AND rewritten.
 * state_dev: the caller zero-fills it to start a fit and passes it back unchanged to continue one.
 * For s = 0 .. n_steps - 1, with no host read in between:
 *   1. stop != 0: loglik_dev[s] = NaN; parameters, state and stationary_dev do not change (the E-step's launches still run, on
 *      the frozen parameters, into the workspace).
 *   2. The E-step on the current parameters: the launches of dff_hmm_estep, statistics and status in the workspace -- its
 *      statistics bit for bit.
 *   3. One launch of one workgroup.  n_estep += 1, estep_status = the E-step's status.  Status != 0: stop = 2, loglik_dev[s] =
 *      NaN, nothing else changes.  Otherwise L = the log-likelihood, loglik_dev[s] = L.  n_estep > 1 and |L - last_loglik| <
 *      accuracy: stop = 1, last_loglik = L, the parameters stay those L was computed with.  Otherwise last_loglik = L and the
 *      M-step, in fp64, every sum in index order from +0, one term after the other, over the m real states:
 *        occ_i = sum_s Gamma[i, s]; B'[i, s] = Gamma[i, s] / occ_i; occ_i <= 0: row i of B is kept, flag bit 0 (also in a step that
 *        ends with stop = 3).  g = sum_i gamma0_i; p0' = gamma0 / g; g <= 0: p0 is kept.
 *        reversible = 0: r_i = sum_j Xi_ij, A'_ij = Xi_ij / r_i; r_i <= 0: row i of A is kept, flag bit 0.
 *        reversible = 1: the graph with an edge i -> j wherever Xi_ij > 0 must be strongly connected over all m states; if not,
 *        stop = 3 and NONE of A, B, p0 changes.  m = 1: A' = [[1]], pi = [1].  Otherwise S = Xi + Xi^T, c_i = sum_j Xi_ij, x_i =
 *        (sum_j S_ij) / 2; a sweep: q_i = c_i / x_i, t_ij = S_ij / (q_i + q_j) where S_ij != 0, else +0, x_i' = sum_j t_ij, err = max_i
 *        |x_i' - x_i| / x_i, x <- x'.  The sweeps end after the first with err < rev_tol, or with an err that is not finite, or
 *        when rev_max_sweeps are spent; rev_max_sweeps spent and the last err not below rev_tol: flag bit 1, x is used anyway.
 *        Then t_ij from the final x, A'_ij = t_ij / x_i, pi = x / sum_i x_i -> stationary_dev; rev_sweeps += the sweeps.
 * The result is a function of the inputs alone: the same from call to call, on any workspace contents, with stationary_dev
 * given or NULL, and n_steps in one call or split over several with the state carried. */
typedef struct {            /* 32 bytes */
    int32_t n_estep;        /* E-steps run so far, over all calls */
    int32_t stop;           /* 0 running | 1 converged | 2 the E-step failed (estep_status) | 3 the reversible estimator's active
                               set lost a hidden state */
    int32_t estep_status;   /* dff_hmm_estep's status word of the last E-step run */
    int32_t flags;          /* bit 0: degenerate (a row kept its previous values); bit 1: a reversible M-step spent
                               rev_max_sweeps without meeting rev_tol */
    double  last_loglik;
    long long rev_sweeps;   /* sweeps of the reversible estimator, all M-steps together */
} dff_hmm_fit_state;
/* Bytes of device workspace the call below needs: dff_hmm_workspace_bytes plus the packed statistics and a status word; -1 on
 * bad arguments. */
long long dff_hmm_fit_workspace_bytes(long long n, const long long* lengths_host, int n_traj, int lag, int m, int K);
int dff_hmm_fit_steps(int device, const int32_t* labels_dev, long long n, const long long* lengths_host, int n_traj, int lag,
                      double* trans_dev /* (m, m) in/out */, double* emit_dev /* (m, K) in/out */, double* init_dev /* (m) in/out */,
                      int m, int K, int reversible, int n_steps, double accuracy, double rev_tol, long long rev_max_sweeps,
                      double* loglik_dev /* (n_steps) */, double* stationary_dev /* (m), written by reversible M-steps only; may be NULL */,
                      dff_hmm_fit_state* state_dev, void* workspace_dev, size_t workspace_bytes, void* stream);

/* ---- Hidden Markov models: the most probable hidden path (Viterbi) of every chain, by a chunked max-plus scan
 * (csrc/dff_hmm_viterbi.hip; evaluate.py: hmm_viterbi_solver, HiddenMarkovModel.viterbi, HmmEvaluator(path="viterbi")) ----
 * Labels, trajectories, chains (r-major, f-minor; chain r lag + f = the frames f, f + lag, ... of trajectory r), chunks
 * (dff_hmm_chunk() frames of a chain), limits and refusals are those of dff_hmm_estep.  The PARAMETERS ARE LOGARITHMS, supplied
 * by the caller, fp64: logtrans_dev (m, m) = la, logemit_dev (m, K) = lb, loginit_dev (m) = lp; -inf is allowed and means an
 * impossible transition, emission or start.  le_t = lb[:, o_t], or zeros for a NEGATIVE label: a missing observation still gets
 * a hidden state.  The device adds, compares and selects, nothing else: no log, no exp, no product.  A max is exact, so the
 * bits follow from the order of the additions, which is this:
 *   (1) per chunk, P = the max-plus identity (0 on the diagonal, -inf elsewhere); for every frame t of the chunk, the chain's
 *       first frame left out:  P'(i, j) = (max_k (P(i, k) + la[k][j])) + le_t(j);
 *   (2) per chain, serially over its chunks: din(first chunk) = lp + le_0, din(next chunk) = dout, dout(j) = max_i (din(i) + P(i, j));
 *   (3) per chunk, from its din, for every frame t of the chunk (the chain's first frame left out):
 *       delta'(j) = (max_i (delta(i) + la[i][j])) + le_t(j), the back-pointer psi_t(j) = the LOWEST i attaining the max; the chunk's
 *       back map origin'(j) = origin(psi_t(j)) from the identity; a chain's last chunk takes the LOWEST argmax of its final delta as
 *       the end state and the max as the chain's log-probability;
 *   (4) per chain, serially from its last chunk: end(c - 1) = origin_c(end(c));  (5) per chunk, from end(c) back through its psi.
 * path_dev (n) int32: the hidden state of every frame, in frame order (chain_order = 0) or in chain order (chain_order = 1: the
 * chains back to back, r-major, f-minor, each in its own time order; the same values, permuted).  chain_logprob_dev (n_traj lag),
 * or NULL: the joint log-probability of every chain's path and labels; an empty chain has 0 and no path entries.
 * status_dev: ONE int32 --
 *   0   success
 *   1   a parameter entry is NaN or +inf
 *   3   a label >= K
 *   2   a non-empty chain whose best path has log-probability -inf (the model cannot emit it)
 * in that order of precedence; on a non-zero status every path entry is -1 and every chain_logprob NaN.
 * What the bits depend on: a chain's path and log-probability follow from that chain's labels, the log-parameters and the chunk
 * length alone -- not from the other chains, the chain's place among them, the lag or trajectory it was cut from, or the workspace.
 * Ties go to the lowest index, for back-pointers and for the end state.  The result is the same from call to call, on any
 * workspace contents, and with chain_logprob_dev given or NULL.  Where every sum is exact in fp64 (integer-valued
 * log-parameters, for example) the path and the log-probability are those of the textbook sequential recursion with the same
 * tie rule; otherwise the carried din differs from the sequential delta by rounding, and with it possibly the choice between
 * paths whose log-probabilities agree to rounding.
 * lag >= 1, n_traj lag <= 2^20 chains, n <= 2^31; device pointers, `stream` only, no read-back, refusals on the host before any
 * device call, no floating-point atomics, no workgroup waits on another.  workspace_dev 8-byte aligned, contents irrelevant. */
/* Bytes of device workspace the call below needs (the trajectory table, the padded log-parameters, per chunk the product, the
 * entering delta, the back map and the end state, per frame one 32-bit word of back-pointers, per chain an end state and a
 * log-probability); -1 on bad arguments. */
long long dff_hmm_viterbi_workspace_bytes(long long n, const long long* lengths_host, int n_traj, int lag, int m, int K);
int dff_hmm_viterbi(int device, const int32_t* labels_dev, long long n, const long long* lengths_host, int n_traj, int lag,
                    const double* logtrans_dev, const double* logemit_dev, const double* loginit_dev, int m, int K,
                    int32_t* path_dev /* (n) */, int chain_order /* 0 frame order, 1 chain order */,
                    double* chain_logprob_dev /* (n_traj lag) or NULL */, int32_t* status_dev,
                    void* workspace_dev, size_t workspace_bytes, void* stream);
/* For benchmarks, process-wide: 0 = the whole call (the default); 1 .. 6 = the call stops after its parameter launch, the chunk
 * products, the forward carries, the apply pass, the backward carries, the backtrack -- the share of every launch, by
 * differences.  The outputs of a call that stopped early are unfinished. */
int dff_debug_hmm_viterbi_stages(int stages);

/* ---- Bootstrap error bars for the Jensen-Shannon metrics: the histogram of every resampling unit, and the JS of B weighted
 * resamples x C channels against a reference histogram (csrc/dff_jsboot.hip; evaluate.py: unit_histograms, bootstrap_js,
 * eval_bootstrap of the evaluators) ----
 * A histogram is additive over frames, so the histogram of resample b is sum_u w[b][u] hist[u]: no frame is looked at again.
 * The conventions of the Markov-model blocks hold: device pointers, `stream` only, no read-back, no synchronisation, refusals on
 * the host before any device call, no floating-point atomics, no workgroup waits on another, bit-identical from call to call,
 * independent of the workspace's prior contents and of how a batch of resamples is split.  Host tables reach the device as
 * kernel arguments.  A channel is one histogram: a bead pair of the PWD metric, or a whole 2-D grid flattened as ix ny + iy.
 * Limits of both calls: 1 <= U <= 65536 units, 1 <= C <= 2^18 channels, 1 <= nbins[c] <= ld <= 2^20, U C ld <= 2^32. */
/* Bytes of device workspace the call below needs (the unit starts and nbins: (U + 1 + C) 64-bit words); -1 on bad arguments. */
long long dff_unit_hist_workspace_bytes(int U, int C);
/* hist_dev[u][c][k] = the number of frames t of unit u with bins_dev[t][c] == k.  bins_dev int32 (n, C): the bin of frame t in
 * channel c; a value < 0 or >= nbins_host[c] is not counted.  unit_lengths_host (U): consecutive units that partition the n
 * frames (zero-length units allowed; they must sum to n).  hist_dev uint32 (U, C, ld) is zeroed by the call, n == 0 included;
 * entries from nbins[c] to ld stay 0.  n <= 2^31.  32-bit integer LDS atomics per workgroup, one workgroup per (unit, channel,
 * tile of 8192 bins), each storing its own slice of the output: exact, whatever nbins[c].  workspace_dev 8-byte aligned. */
int dff_unit_hist(int device, const int32_t* bins_dev, long long n, int C, const long long* unit_lengths_host, int U,
                  const int32_t* nbins_host, int ld, uint32_t* hist_dev, void* workspace_dev, size_t workspace_bytes, void* stream);
/* Bytes of device workspace the call below needs: nbins, the units' channel totals and the reference sums, (C + U C + C) 64-bit
 * words.  It does not depend on B or ld: no resampled histogram is ever written to memory.  -1 on bad arguments. */
long long dff_resampled_js_workspace_bytes(int U, int C);
/* js_dev[b][c] = the Jensen-Shannon divergence between resample b's histogram of channel c and the reference's.  hist_dev uint32
 * (U, C, ld) as dff_unit_hist writes it (counts summing to at most 2^31 per channel); weights_dev uint32 (B, U), the
 * multiplicity of unit u in resample b; ref_dev fp64 (C, ld), counts or densities, not normalised.  For k < nbins[c]:
 *   h[k] = sum_u w[b][u] hist[u][c][k]    (uint64, exact: no sum can overflow)
 *   tot = sum_k h[k],   p[k] = h[k] / tot + 1e-10,   q[k] = ref[c][k] / sum_k ref[c][k] + 1e-10,   m = (p + q) / 2
 *   js[b][c] = 1/2 sum_k ( p ln(p / m) + q ln(q / m) )
 * in fp64: the reference's js_divergence.  The sum over k is taken in one order that depends on nbins[c] alone (thread t of 256
 * adds bins t, t + 256, ... in ascending order, the threads are added by a butterfly per wave and the four waves as
 * (0 + 1) + (2 + 3)), likewise sum_k ref.  js is NaN, and confined to that (b, c), when tot == 0, when sum_k ref[c] is 0 or not
 * finite, or when an entry of ref[c] is negative or not finite.  total_dev uint64 (B, C), may be NULL: tot, exact.
 * 1 <= B <= 4096.  One workgroup per (channel, tile of 1, 2, 4 or 8 resamples), threads along the bins, the tile's weights in
 * LDS, one 32 x 32 -> 64 multiply-add per (b, u, k).  workspace_dev 8-byte aligned, contents irrelevant. */
int dff_resampled_js(int device, const uint32_t* hist_dev, int U, int C, int ld, const int32_t* nbins_host,
                     const uint32_t* weights_dev, int B, const double* ref_dev, double* js_dev, uint64_t* total_dev,
                     void* workspace_dev, size_t workspace_bytes, void* stream);
/* Host only: the resamples per workgroup a call with B resamples and C channels would take now (the power of two that holds min(B, 8),
 * halved until the call has 512 workgroups, at least 1); -1 on bad arguments. */
int dff_resampled_js_path_for(int B, int C);
/* For tests and benchmarks, process-wide: 0 = the tile follows (B, C) (the default); 1, 2, 4 or 8 = that many resamples per
 * workgroup.  Every tile gives the same bits. */
int dff_debug_resampled_js_path(int path);

const char* dff_last_error(void);
const char* dff_version(void);

#ifdef __cplusplus
}
#endif
#endif /* DFF_H */
