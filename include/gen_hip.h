/* gen_hip.h — C ABI of libgen_hip.so, the MI355X particle-inference engine.
 *
 * This is the drop-in boundary for Gen's sequential-Monte-Carlo hot path.
 * The reference has no FFI: its interface is Julia multiple dispatch on
 * `ParticleFilterState{U}` and the generative-function interface (GFI).  Each
 * entry point below replaces one reference function; the Julia `ccall`
 * binding a maintainer adds is spelled out in INTEGRATION.md.
 *
 *   gh_pf_init              initialize_particle_filter   src/inference/particle_filter.jl:79-108
 *   gh_pf_step              particle_filter_step!        src/inference/particle_filter.jl:139-180
 *   gh_pf_maybe_resample    maybe_resample!              src/inference/particle_filter.jl:189-213
 *   gh_pf_log_ml_estimate   log_ml_estimate              src/inference/particle_filter.jl:52-55
 *   gh_pf_get_log_weights   get_log_weights              src/inference/particle_filter.jl:43-45
 *   gh_pf_get_states /
 *   gh_pf_get_trajectory    get_traces (SoA columns)     src/inference/particle_filter.jl:31-34
 *   gh_pf_get_parents       ParticleFilterState.parents  src/inference/particle_filter.jl:23
 *   gh_pf_estimate          effective_sample_size /      src/inference/particle_filter.jl:3-14, and
 *                           normalize_weights            the expectation callers take over get_traces
 *                                                        with get_log_weights
 *   gh_pf_quantiles         the weighted median and      src/inference/particle_filter.jl:31-45: the sort
 *                           credible band of get_traces  per component callers run over get_traces with
 *                           under get_log_weights        get_log_weights (normalize_weights, :8-14)
 *   gh_pf_estimate_path /
 *   gh_pf_quantiles_path    the same expectation and the src/inference/particle_filter.jl:31-45, for
 *                           same sort, for every step    every step of the Unfold: the loop callers run
 *                           of get_traces at once        over the steps of get_traces with get_log_weights
 *   gh_pf_forecast          particle_filter_step! with   src/inference/particle_filter.jl:139-160 on a
 *                           EmptyChoiceMap() on a copy   copy of the state; the Unfold extended by
 *                           of the state, k = 1..H, and  update with no constraints
 *                           :y drawn as simulate does    (src/modeling_library/unfold/update.jl:54-78);
 *                                                        :y as src/static_ir/simulate.jl:23-34
 *   gh_pf_get_log_weights_at get_log_weights as it stood  src/inference/particle_filter.jl:43-45 at every
 *                           after step t                 step: log_weights before maybe_resample! resets
 *                                                        them (:189-213)
 *   gh_pf_backward_weights  log_weights of step t plus   src/inference/particle_filter.jl:43-45 and the
 *                           the score of :x at t + 1     Unfold kernel's :x score
 *                                                        (src/static_ir/trace.jl:91-129)
 *   gh_pf_smooth            backward simulation over     Gen has no smoother: a caller would loop over
 *                           get_traces and the recorded  get_traces and get_log_weights kept per step
 *                           log_weights (FFBSi)          (src/inference/particle_filter.jl:31-45) and
 *                                                        draw as categorical does, as
 *                                                        sample_unweighted_traces (:62-70) does at T
 *   gh_pf_get_scores        get_score / per-choice scores src/static_ir/trace.jl:91-129
 *   gh_pf_sample_unweighted sample_unweighted_traces     src/inference/particle_filter.jl:62-70
 *   gh_pf_rejuvenate        mh(trace, select(x_t)) on    src/inference/mh.jl:14-26 (applied per
 *                           every particle               particle, as callers of the PF do)
 *   gh_pf_mh_select         mh(trace, selection) on      src/inference/mh.jl:14-28,
 *                           every particle               examples/regression/quickstart.jl:17-22
 *   gh_pf_mh_drift          mh(trace, drift, (sd,)) on   src/inference/mh.jl:41-62 (proposal form)
 *                           every particle
 *   gh_pf_choice_gradients  choice_gradients(trace,      src/gen_fn_interface.jl:374-406,
 *                           selection) on every particle src/static_ir/backprop.jl
 *   gh_pf_mala              mala(trace, selection, tau)  src/inference/mala.jl:11-54
 *                           on every particle
 *   gh_pf_hmc               hmc(trace, selection; L,     src/inference/hmc.jl:25-72
 *                           eps) on every particle
 *   gh_pf_elliptical_slice  elliptical_slice(trace, addr, src/inference/elliptical_slice.jl:13-45
 *                           mu, cov) on every particle   (the likelihood-only slice, see below)
 *   gh_pf_map_optimize      map_optimize(trace,          src/inference/map_optimize.jl:9-41
 *                           selection) on every particle
 *   gh_pf_init_conditional /
 *   gh_pf_step_conditional  conditional_smc              examples/pmmh/smc.jl:100-151
 *     with gh_pf_opts       the same sweep, the          smc.jl:136-139 fix that parent (parents[ONE] = ONE);
 *     .ancestor_sampling    distinguished particle's     the draw is PGAS's (Lindsten, Jordan & Schon 2014),
 *                           parent drawn                 which Gen does not have
 *   gh_is_run               importance_sampling          src/inference/importance.jl:20-52
 *   gh_pmmh_run             PMMH (mh over a PF-estimated  examples/pmmh/example.jl:20-79,
 *                           likelihood)                   examples/pmmh/pf.jl:14-73
 *   gh_coal_run             involutive (RJ) MH chains     examples/coal/coal.jl:126-336,
 *                                                         src/inference/mh.jl:85-98
 *   gh_simulate             simulate(model, (T,)) for N  src/static_ir/simulate.jl:23-34,50-83,
 *                           traces                       src/modeling_library/unfold/simulate.jl
 *   gh_dist_logpdf /        logpdf / random of the       src/modeling_library/modeling_library.jl:15-41,
 *   gh_dist_random          distribution library         src/modeling_library/distributions/ (all files)
 *   gh_model_create         a Static-DSL model + Unfold  src/static_ir/, src/modeling_library/unfold/
 *
 * Conventions
 *  - Every function returns an int status (GH_OK = 0); the message of the
 *    last failure on this thread is gh_last_error().  Julia's `error(...)`
 *    sites map to status codes (see gh_status).
 *  - Handles are opaque; the library owns all device memory.  Host inputs are
 *    copied at call time, outputs are written into caller-allocated buffers.
 *  - Particle indices are 0-based (Julia's are 1-based).
 *  - A gh_pf is driven by one host thread (as the reference's mutable state is);
 *    distinct handles may run concurrently on distinct streams.  The resample
 *    kernels synchronise their whole grid (sized to the co-resident capacity of
 *    an idle device, no cooperative launch: it costs ~16 us per step), so they
 *    assume no other kernel occupies the GPU while they run.  If blocks are
 *    not co-resident the bounded barrier wait expires, the kernel writes
 *    nothing and the next synchronising call returns GH_E_STATE.
 *  - Multi-GPU: one process per GPU.  Create the context with
 *    gh_ctx_create_dist(); particles [rank*n/world, (rank+1)*n/world) live on
 *    each rank and every gh_pf_* call is collective over the ranks.
 */
#ifndef GEN_HIP_H
#define GEN_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GH_OK = 0,
  GH_E_INVAL = 1,    /* bad argument (cf. unfold.jl:57-61 negative length, vector.jl:110) */
  GH_E_DISCARD = 2,  /* a constraint hit an existing choice inside a PF step (particle_filter.jl:168-170) */
  GH_E_NUMERIC = 3,  /* all log-weights -Inf / NaN (Categorical with NaN probabilities) */
  GH_E_NOMEM = 4,
  GH_E_HIP = 5,
  GH_E_RCCL = 6,
  GH_E_STATE = 7     /* call out of order (e.g. step before init); resample grid barrier timed out */
} gh_status;

typedef enum {
  /* x_1 ~ mvnormal(mu0, P0); x_t ~ mvnormal(A x_{t-1} + b, Q); y_t ~ mvnormal(H x_t + c, R)
     params (row-major doubles): A[d*d] b[d] Q[d*d] H[dy*d] c[dy] R[dy*dy] mu0[d] P0[d*d]
     supported d: 1..16; dy <= 32.  Multi-rank filters use systematic resampling. */
  GH_FAMILY_LGSSM = 1,
  /* categorical HMM (test/inference/particle_filter.jl:50-78):
     z_1 ~ categorical(prior); z_t ~ categorical(T[:, z_{t-1}]); x_t ~ categorical(E[:, z_t])
     params: prior[k] T[k*k] (T[new*k + prev]) E[v*k] (E[x*k + z]); k <= 64 */
  GH_FAMILY_HMM = 2,
  /* nonlinear "Kitagawa" SSM (examples/pmmh/model.jl:9-13,40-46):
     x_1 ~ normal(mu1, s1); x_t ~ normal(x/2 + 25x/(1+x^2) + 8cos(1.2t), sqrt(var_x));
     y_t ~ normal(x_t^2/20, sqrt(var_y));  params: mu1 s1 var_x var_y */
  GH_FAMILY_KITAGAWA = 3,
  /* Bayesian linear regression (examples/regression/quickstart.jl:3-9), a static
     model (generate / importance sampling / rejuvenation; no steps):
     slope ~ normal(mu_s, sd_s); intercept ~ normal(mu_i, sd_i);
     y_i ~ normal(slope x_i + intercept, sigma), i = 1..dy (dy <= 32 data points)
     params: mu_s sd_s mu_i sd_i sigma x[dy]; the observation is y[dy];
     state (d = 2) = (slope, intercept) */
  GH_FAMILY_REGRESSION = 4,
  /* slot-described Unfold kernel (Static-DSL models other than the four
     above, static_ir/generate.jl:24-43): one latent address and K = 1..4
     observed addresses ("slots") per step, any subset of which a step
     constrains (gh_obs.slot / .next).  d (latent dimension) 1..16.
       params = [lat, K, (dist_k, m_k, link_k) for k < K, latent block, slot blocks]
     latent block, lat = GH_SLOT_LAT_AFFINE (0):   A[d*d] b[d] Q[d*d] mu0[d] P0[d*d]
         x_1 ~ mvnormal(mu0, P0); x_t ~ mvnormal(A x_{t-1} + b, Q)
                   lat = GH_SLOT_LAT_AFFINE_INPUT (2): the same block, and
         x_t ~ mvnormal(A x_{t-1} + (b + u_t), Q) with u_t the step's input (a
         gh_obs entry with slot GH_SLOT_INPUT and d values; zero when a step
         gives none): the Unfold's kernel arguments extended by one value per
         step, new_args = (t, u_t) (no re-scoring: earlier steps keep theirs);
         simulate(model, (T, U)) is gh_simulate_inputs (gh_simulate refuses)
                   lat = GH_SLOT_LAT_KITAGAWA (1), d = 1: mu1 s1 sd_x
         x_1 ~ normal(mu1, s1); x_t ~ normal(x/2 + 25x/(1+x^2) + 8cos(1.2t), sd_x)
                   lat = GH_SLOT_LAT_CATEGORICAL (3), d = K classes (2..16): prior[K] T[K*K]
         z_1 ~ categorical(prior); z_t ~ categorical(T[:, z_{t-1}]) (T[new*K + prev]);
         the state is stored one-hot (K values), so a slot's affine mean h.x + c
         is h[z] + c (per-class parameters); no drift MH, no linear proposal
                   lat = GH_SLOT_LAT_SWITCHING (4), two latent addresses, d = dx + nz:
         nz (2..8) prior[nz] T[nz*nz], per regime A_z[dx*dx] b_z[dx] Q_z[dx*dx], mu0[dx] P0[dx*dx]
         z_1 ~ categorical(prior), x_1 ~ mvnormal(mu0, P0); z_t ~ categorical(T[:, z_{t-1}]),
         x_t ~ mvnormal(A_z x_{t-1} + b_z, Q_z) with z = z_t; the state is x (dx values) then
         z one-hot (nz values), so a slot's h.x + c loads x and adds h[dx + z];
         no drift MH, no linear proposal, MH selections name both addresses
     slot blocks (m_k values of the slot; its value rows in simulate's output
     follow slot order, one row for a scalar slot):
       GH_SLOT_MVNORMAL, link GH_LINK_AFFINE, m <= 32: H[m*d] c[m] R[m*m]   y ~ mvnormal(H x + c, R)
       GH_SLOT_NORMAL, m = 1, GH_LINK_AFFINE: h[d] c sd                     y ~ normal(h.x + c, sd)
                              GH_LINK_KITAGAWA (d = 1): sd                  y ~ normal(x^2/20, sd)
                              GH_LINK_LOGSCALE: h[d] c g[d] s   y ~ normal(h.x + c, exp(g.x + s))
         (a log-linear standard deviation: the stochastic-volatility emission
         y_t ~ normal(0, exp(x_t / 2)) is h = 0, c = 0, g = 1/2, s = 0)
       GH_SLOT_POISSON, m = 1, GH_LINK_EXP: h[d] c                         y ~ poisson(exp(h.x + c))
       GH_SLOT_BERNOULLI, m = 1, GH_LINK_LOGISTIC: h[d] c   y ~ bernoulli(1 / (1 + exp(-(h.x + c)))) (0 / 1)
       GH_SLOT_CATEGORICAL, m = classes 2..16, GH_LINK_SOFTMAX: W[m*d] c[m]
                                     y ~ categorical(softmax(W x + c)), 0-based class
       GH_SLOT_LIBRARY, m = a scalar distribution of Gen's library by its
         gh_dist_desc id (GH_DIST_NORMAL, _UNIFORM_CONTINUOUS, _UNIFORM_DISCRETE,
         _BERNOULLI, _GAMMA, _INV_GAMMA, _BETA, _EXPONENTIAL, _POISSON, _BINOMIAL,
         _NEG_BINOMIAL, _GEOMETRIC, _LAPLACE, _CAUCHY, _BETA_UNIFORM), link 0:
         per argument (Gen's order) link_j h_j[d] c_j, the argument being
         link_j(h_j.x + c_j) with link_j GH_ARG_IDENTITY, GH_ARG_EXP or
         GH_ARG_LOGISTIC; y ~ dist(args...) scored by the library's logpdf
         (gh_dist_logpdf's formulas) and drawn by its sampler in simulate
     Optional trailing block, dependencies between a step's observed addresses:
       nd, then nd triples (child k, parent j < k, g): the child's linear
       predictor (a normal slot's affine mean, a poisson / bernoulli slot's
       h.x + c, a library slot's first argument) adds the fma chain of g * y_j
       over its parents in slot order; parents are scalar slots; a step that
       constrains a child constrains its parents (else GH_E_INVAL); simulate
       draws the parents first.
     At most 32 observed values per step (a poisson slot counts 2).  An LGSSM
     or Kitagawa model written as slots filters bit for bit as its family does
     (those stay the fast paths); the default proposal or GH_PROPOSAL_LINEAR
     (d + observed values <= 32); gh_pf_step_params takes a new slot model
     with the same latent form and slot layout (only the numbers change). */
  GH_FAMILY_SLOTS = 5
} gh_family;

enum { GH_SLOT_LAT_AFFINE = 0, GH_SLOT_LAT_KITAGAWA = 1, GH_SLOT_LAT_AFFINE_INPUT = 2, GH_SLOT_LAT_CATEGORICAL = 3,
       GH_SLOT_LAT_SWITCHING = 4 };
/* gh_obs.slot of a step's latent input u_t (latent form 2): d values, an
   argument of the step's kernel application, not a choice */
enum { GH_SLOT_INPUT = -1 };
enum { GH_SLOT_MVNORMAL = 1, GH_SLOT_NORMAL = 2, GH_SLOT_POISSON = 3, GH_SLOT_BERNOULLI = 4, GH_SLOT_CATEGORICAL = 5,
       GH_SLOT_LIBRARY = 6 };
enum { GH_ARG_IDENTITY = 0, GH_ARG_EXP = 2, GH_ARG_LOGISTIC = 3 };  /* a library slot's argument links */
enum { GH_LINK_AFFINE = 0, GH_LINK_KITAGAWA = 1, GH_LINK_EXP = 2, GH_LINK_LOGISTIC = 3, GH_LINK_SOFTMAX = 4,
       GH_LINK_LOGSCALE = 5 };

typedef enum { GH_RESAMPLE_SYSTEMATIC = 0, GH_RESAMPLE_MULTINOMIAL = 1 } gh_resampler;

typedef enum {
  GH_PROPOSAL_DEFAULT = 0, /* the model's internal proposal (prior) */
  GH_PROPOSAL_OPTIMAL = 1, /* locally optimal proposal p(x_t | x_{t-1}, y_t) as a custom
                              proposal (particle_filter.jl:79-91,139-154): HMM (the proposal
                              of test/inference/particle_filter.jl:104-127) and LGSSM
                              (Gaussian, d + dy <= 32); weight log p(y_t | x_{t-1}) */
  GH_PROPOSAL_GAUSSIAN = 2 /* user-parameterised custom proposal of the nonlinear SSM
                              (particle_filter.jl:79-91,139-154 via trace_translators.jl:
                              775-802): x_t ~ normal(alpha m + beta y_t + gamma, sigma_q),
                              m the prior mean; proposal_args = (alpha, beta, gamma, sigma_q)
                              through gh_pf_init_q / gh_pf_step_q; weight log p(x_t|x_{t-1})
                              + log p(y_t|x_t) - log q(x_t) */,
  GH_PROPOSAL_LINEAR = 3  /* user-parameterised custom proposal of the LGSSM and of slot models (the same
                              translator): x_t ~ mvnormal(P x_{t-1} + u_t, Sigma_q) (t = 1:
                              mvnormal(u_1, Sigma_q)); proposal_args = P[d*d] Sigma_q[d*d] u[d]
                              (required at gh_pf_init_q), or u[d] alone to keep P and Sigma_q
                              (none: keep u too); d + dy <= 32; weight log p(x_t|x_{t-1})
                              + log p(y_t|x_t) - log q(x_t) */
} gh_proposal;

typedef struct gh_ctx gh_ctx;
typedef struct gh_model gh_model;
typedef struct gh_pf gh_pf;

typedef struct {
  int32_t family; /* gh_family */
  int32_t d;      /* latent dimension (LGSSM) */
  int32_t dy;     /* observation dimension (LGSSM) */
  int32_t k;      /* number of hidden states (HMM) */
  int32_t v;      /* number of observation symbols (HMM) */
  const double* params;
  int64_t n_params;
} gh_model_desc;

/* The observations of one step: the value(s) at address :chain => t => :y.
   values == NULL or present == 0 means "no observation at this step".
   GH_FAMILY_SLOTS: `slot` names the observed address (0..K-1) and `next`
   chains the step's other constrained addresses (NULL ends the chain; a
   slot constrained twice is GH_E_DISCARD); an entry with slot
   GH_SLOT_INPUT (-1) carries the step's latent input u_t (latent form 2, d
   values, at most one per step); the other families take slot 0 and no
   chain. */
typedef struct gh_obs {
  const double* values;
  int32_t n_values;
  int32_t present;
  int32_t slot;
  int32_t reserved;
  const struct gh_obs* next;
} gh_obs;

typedef struct {
  int32_t resampler;      /* gh_resampler */
  int32_t record_history; /* 1: keep every step's states + genealogy (Gen trace semantics) */
  int32_t history_capacity; /* steps to preallocate when record_history (0 = grow) */
  int32_t block_size;     /* 0 = default (256) */
  int32_t time_kernels;   /* k > 0: time every k-th step kernel with hipEvents (gh_pf_kernel_time) */
  int32_t record_weights; /* 1: keep every step's log-weights too (needs record_history): one device-to-device
                             copy of n doubles per step; what gh_pf_backward_weights and gh_pf_smooth read */
  int32_t ancestor_sampling; /* 1: a conditional filter (gh_pf_init_conditional) draws the distinguished
                                particle's parent at every step whose resample fired (see gh_pf_step_conditional) */
  int32_t reserved;
} gh_pf_opts;

/* ---- context ------------------------------------------------------------ */
int gh_ctx_create(int device, void* hip_stream /* NULL = own stream */, gh_ctx** out);
int gh_comm_unique_id(uint8_t id[128]);
int gh_ctx_create_dist(int device, int rank, int world, const uint8_t id[128], void* hip_stream,
                       gh_ctx** out);
/* Host-staged transport (e.g. several ranks sharing one GPU, or a cluster
   without RCCL peer access): the library stages device buffers through host
   memory and calls these functions, which move host buffers between ranks.
   Return 0 on success. */
typedef struct {
  void* user;
  /* every rank contributes `bytes`; recv receives world*bytes in rank order */
  int (*allgather)(void* user, const void* send, void* recv, uint64_t bytes);
  /* point-to-point exchange: the calls of all ranks match pairwise */
  int (*sendrecv)(void* user, int n_send, const int* send_peers, const void* const* send_bufs,
                  const uint64_t* send_bytes, int n_recv, const int* recv_peers, void* const* recv_bufs,
                  const uint64_t* recv_bytes);
} gh_host_comm;
int gh_ctx_create_hostcomm(int device, int rank, int world, const gh_host_comm* comm, void* hip_stream,
                           gh_ctx** out);
/* Peer transport: the ranks' kernels exchange through device memory they map
   from each other (a fine-grained mailbox per rank, and every filter's
   received-row buffer), with tagged words and bounded polls — no collective
   call and no host round trip on the step path.  The bootstrap's allgather
   (host buffers) swaps the IPC handles once, at context and filter creation
   (both collective over the ranks, and fail-together: a rank that fails its
   part makes every rank's call return an error, none is left waiting), and
   fences the ranks at gh_ctx_destroy and at gh_pf_destroy of a multi-rank
   filter — on this transport both destroys are COLLECTIVE: every rank calls
   them, in the same order.  Ranks on one GPU (processes sharing a device) or
   on GPUs that map each other's memory (xGMI peers of one node).
   world <= 64.  Systematic resampling moves its rows inside the fused
   kernels; the other forms (multinomial, conditional SMC, the generic
   exchange) move theirs through the bootstrap's sendrecv when it is given
   (GH_E_STATE without it).  Every device wait on another rank is bounded
   in time (gh_ctx_set_peer_timeout, 30 s by default): a rank that stops
   posting makes the others' waits end in GH_E_STATE ("peer transport: ...");
   a slow one is waited for. */
int gh_ctx_create_peer(int device, int rank, int world, const gh_host_comm* bootstrap, void* hip_stream,
                       gh_ctx** out);
/* the bound of every device wait on another rank (peer transport; later
   launches), seconds in (0, 86400]; no effect on the other transports */
int gh_ctx_set_peer_timeout(gh_ctx* ctx, double seconds);
int gh_ctx_destroy(gh_ctx* ctx);
/* Debug / timing: filters created on this context afterwards take the
   multi-rank code path (collectives, split step after a resample, k_rank_a/b)
   even at world 1 — over a one-rank RCCL communicator for a gh_ctx_create /
   gh_ctx_create_dist context, over the user's functions for a host-comm one.
   Results are the same filter's (bit-exact against the one-rank path).
   GH_E_STATE while a filter exists on the context (its buffers were
   allocated for the path chosen when it was created). */
int gh_ctx_force_multirank(gh_ctx* ctx);
int gh_ctx_rank(const gh_ctx* ctx, int* rank, int* world);
int gh_ctx_stream(const gh_ctx* ctx, void** hip_stream);
int gh_ctx_synchronize(gh_ctx* ctx);

/* ---- models --------------------------------------------------------------- */
int gh_model_create(gh_ctx* ctx, const gh_model_desc* desc, gh_model** out);
int gh_model_destroy(gh_model* m);
int gh_model_state_dim(const gh_model* m, int* d);
/* simulate(model, (T,)) n times (static_ir/simulate.jl:23-34: every choice
   sampled from its distribution, score += logpdf of the sampled value; the
   Unfold runs its kernel T times).  Trace i draws from (seed, i, t, simulate
   stream), independent of n.  Outputs (host, each nullable, time-major):
     xs[t-1][k][i]        latent component k of :chain => t => :x (regression: slope, intercept)
     ys[t-1][r][i]        observation component r of :chain => t => :y (HMM: the symbol;
                          regression: y-(r+1)); r < dy (1 for HMM and Kitagawa)
     per_step[t-1][0|1][i] the latent's / the observation's score
     total[i]             get_score(trace i), the scores summed in time order
   The regression model takes T = 1. */
int gh_simulate(gh_model* m, int T, int64_t n, uint64_t seed, double* xs, double* ys, double* per_step,
                double* total);
/* simulate(model, (T, U)) for a slot model with per-step inputs (latent form
   2; gh_simulate refuses one): inputs[T*d], row t-1 the input u_t of step t
   (row 0 unused); outputs as gh_simulate. */
int gh_simulate_inputs(gh_model* m, int T, int64_t n, uint64_t seed, const double* inputs, double* xs, double* ys,
                       double* per_step, double* total);

/* ---- distributions ----------------------------------------------------------- */
/* Gen's distribution library (src/modeling_library/distributions/), batched:
   n values, one parameter row shared by all (param_stride 0) or one row per
   value (param_stride = n_params).  Parameter rows, in Gen's argument order:
     NORMAL mu std | BROADCASTED_NORMAL mu[dim] std[dim] | MVNORMAL mu[dim] cov[dim*dim]
     UNIFORM_CONTINUOUS low high | UNIFORM_DISCRETE low high | BERNOULLI prob
     CATEGORICAL probs[K] (K = n_params) | GAMMA shape scale | INV_GAMMA shape scale
     BETA alpha beta | EXPONENTIAL rate | POISSON lambda | BINOMIAL n p
     NEG_BINOMIAL r p | GEOMETRIC p | LAPLACE loc scale | CAUCHY x0 gamma
     PIECEWISE_UNIFORM bounds[K+1] probs[K] | BETA_UNIFORM theta alpha beta
   Values are doubles, component-major [dim][n] for the vector distributions;
   integer values are stored exactly, bernoulli is 0/1, categorical is 1-based
   (as Gen's).  random(): value i draws from the Philox stream keyed
   (seed, i), independent of n.  The *_dev forms take device x / out and
   enqueue on the context's stream (params_on_device: params is a device
   pointer; not for MVNORMAL, whose Cholesky factor is taken on the host). */
typedef enum {
  GH_DIST_NORMAL = 1, GH_DIST_BROADCASTED_NORMAL = 2, GH_DIST_MVNORMAL = 3, GH_DIST_UNIFORM_CONTINUOUS = 4,
  GH_DIST_UNIFORM_DISCRETE = 5, GH_DIST_BERNOULLI = 6, GH_DIST_CATEGORICAL = 7, GH_DIST_GAMMA = 8,
  GH_DIST_INV_GAMMA = 9, GH_DIST_BETA = 10, GH_DIST_EXPONENTIAL = 11, GH_DIST_POISSON = 12, GH_DIST_BINOMIAL = 13,
  GH_DIST_NEG_BINOMIAL = 14, GH_DIST_GEOMETRIC = 15, GH_DIST_LAPLACE = 16, GH_DIST_CAUCHY = 17,
  GH_DIST_PIECEWISE_UNIFORM = 18, GH_DIST_BETA_UNIFORM = 19
} gh_dist;

typedef struct {
  int32_t dist;             /* gh_dist */
  int32_t dim;              /* value components (BROADCASTED_NORMAL, MVNORMAL); else 1 */
  int32_t n_params;         /* doubles per parameter row */
  int32_t param_stride;     /* 0: one shared row; n_params: row i for value i */
  int32_t params_on_device; /* *_dev forms: params is a device pointer */
  int32_t reserved;
  const double* params;
} gh_dist_desc;

int gh_dist_logpdf(gh_ctx* ctx, const gh_dist_desc* d, int64_t n, const double* x /* [dim][n] */,
                   double* out /* [n] */);
int gh_dist_random(gh_ctx* ctx, const gh_dist_desc* d, int64_t n, uint64_t seed, double* out /* [dim][n] */);
int gh_dist_logpdf_dev(gh_ctx* ctx, const gh_dist_desc* d, int64_t n, const double* x, double* out);
int gh_dist_random_dev(gh_ctx* ctx, const gh_dist_desc* d, int64_t n, uint64_t seed, double* out);

/* ---- particle filter -------------------------------------------------------- */
void gh_pf_opts_default(gh_pf_opts* o);
int gh_pf_init(gh_model* m, const gh_obs* obs, int proposal, int64_t n_particles, uint64_t seed,
               const gh_pf_opts* opts, gh_pf** out);
int gh_pf_destroy(gh_pf* pf);  /* collective for a multi-rank filter on the peer transport */
int gh_pf_step(gh_pf* pf, const gh_obs* obs, int proposal);
/* initialize_particle_filter(model, args, obs, proposal, proposal_args, N) and
   particle_filter_step!(state, args, argdiffs, obs, proposal, proposal_args)
   (particle_filter.jl:79-91, 139-154) for proposals with arguments
   (GH_PROPOSAL_GAUSSIAN: 4 doubles).  The arguments are kept: gh_pf_step and
   gh_pf_run reuse the last ones given. */
int gh_pf_init_q(gh_model* m, const gh_obs* obs, int proposal, const double* proposal_args, int n_proposal_args,
                 int64_t n_particles, uint64_t seed, const gh_pf_opts* opts, gh_pf** out);
int gh_pf_step_q(gh_pf* pf, const gh_obs* obs, int proposal, const double* proposal_args, int n_proposal_args);
/* particle_filter_step!(state, (t, params'...), (UnknownChange(), UnknownChange()...),
   observations) (particle_filter.jl:162-180) with the Unfold's parameters
   changed to those of new_model (same family and dimensions, same context):
   the Unfold's update re-visits every retained kernel application
   (unfold/generic_update.jl:9-16), so every particle's weight gains its
   trajectory's score under the new parameters minus under the old ones, and
   the new step is generated under the new parameters, which the filter keeps
   from then on (new_model must outlive it).  record_history; on R ranks
   every rank calls it (the re-scoring walks the genealogy across ranks). */
int gh_pf_step_params(gh_pf* pf, const gh_obs* obs, int proposal, gh_model* new_model);
/* The same for a conditional filter (gh_pf_init_conditional): the re-scoring,
   then the conditional step of gh_pf_step_conditional with the distinguished
   particle pinned to ref_xt[d] (particle Gibbs with a parameter move between
   sweeps, examples/pmmh/smc.jl:138-147).  The reference's Unfold update KAT
   with changed parameters (test/modeling_library/unfold.jl:303-326) is driven
   through this entry: tests/test_step_params.py. */
int gh_pf_step_params_conditional(gh_pf* pf, const gh_obs* obs, gh_model* new_model, const double* ref_xt);
/* ess_threshold NaN means the reference's default N/2; any other value >= 0 is
   the threshold as given (resample iff ESS < ess_threshold, so 0 never
   resamples, as in Gen); a negative threshold is GH_E_INVAL (before round 3,
   values <= 0 selected N/2).  If did_resample/ess are non-NULL the
   call synchronises and reports them; otherwise the decision stays on the
   device and the call is asynchronous. */
int gh_pf_maybe_resample(gh_pf* pf, double ess_threshold, int* did_resample, double* ess);
/* run {maybe_resample!; particle_filter_step!} for n_steps consecutive steps
   (the reference caller loop, test/inference/particle_filter.jl:157-162),
   observations obs[0..n_steps-1]; no host synchronisation inside. */
int gh_pf_run(gh_pf* pf, int n_steps, const gh_obs* obs, int proposal, double ess_threshold);
int gh_pf_log_ml_estimate(gh_pf* pf, double* out);
int gh_pf_num_particles(const gh_pf* pf, int64_t* n_global, int64_t* n_local, int64_t* first);
int gh_pf_num_steps(const gh_pf* pf, int* t);
int gh_pf_get_log_weights(gh_pf* pf, double* host_out /* n_local */);
int gh_pf_get_states(gh_pf* pf, double* host_out /* [d][n_local] current latent */);
int gh_pf_get_parents(gh_pf* pf, int64_t* host_out /* n_local, global ids */);
/* latent of step t (1-based) of the current particles' traces: follows the
   genealogy back from the current step (record_history required) */
int gh_pf_get_trajectory(gh_pf* pf, int t, double* host_out /* [d][n_local] */);
/* The effective sample size and the weighted mean and covariance of the
   current particles, reduced on the device: only the outputs asked for leave
   it (at most 1 + d + d^2 doubles, one synchronise).  With w_i = exp(lw_i -
   max lw), W = sum w_i and x_i the latent of step t of particle i's trace
   (t = 0: the current step; 1 <= t <= the current step: along the genealogy,
   as gh_pf_get_trajectory, record_history required for an earlier step):
     ess      = W^2 / sum w_i^2
     mean[k]  = sum w_i x_ik / W
     cov[k][l] = sum w_i (x_ik - mean[k]) (x_il - mean[l]) / W
   cov is the weighted POPULATION covariance (no Bessel correction), full,
   row-major and exactly symmetric.  The estimate is of the stored doubles:
   for a categorical latent it is the mean of the class index.  A particle of
   weight exactly 0 adds nothing, whatever its state.  While a resample is
   pending the particles are the resampled ones with equal weights (ess = n),
   as gh_pf_get_states and gh_pf_get_log_weights report them.  Any of ess,
   mean, cov may be NULL (all three NULL: GH_E_INVAL); ess alone runs no pass
   over the particles, mean one, cov two (centred on the first pass's mean).
   Log-weights all -inf, or holding a NaN: GH_E_NUMERIC.  One rank only: a
   filter on the multi-rank path returns GH_E_STATE.  Every model family.
   Deterministic: the same filter gives the same bits. */
int gh_pf_estimate(gh_pf* pf, int t, double* ess /* 1 */, double* mean /* [d] */, double* cov /* [d][d] */);
/* Weighted quantiles of the current particles, per component, selected on the
   device: out[j][k] = Q_k(probs[j]); n_probs x d doubles leave it, after one
   synchronise.  The definition is on the resampler's integer weights, so it
   is exact and the same bits on every run.  With n the particle count, x_i
   the latent of step t along particle i's genealogy (gh_pf_estimate's meaning
   of t, 0 = the current step), lw_i its log-weight and M = max lw:
     shift = 62 - ceil(log2 n), at most 52          (the resampler's)
     q_i   = floor(exp(lw_i - M) 2^shift)           an unsigned integer; lw_i = -inf: 0
     S     = sum q_i
   and for a probability p in [0, 1]
     u     = floor(p 2^53)                          exact in fp64
     r     = max(1, ceil(u S / 2^53))               exact integer arithmetic; p = 1: r = S
   While a resample is pending the particles are the resampled ones and every
   q_i = 2^shift: the particles and weights gh_pf_estimate uses.  Doubles are
   ordered by the total-order key, the bit pattern with all bits flipped for
   negatives and the sign bit flipped otherwise: -0.0 < +0.0, and a NaN state
   sorts by its bits and is not refused.  Then
     Q_k(p) = the smallest v among {x_ik : q_i > 0} with sum_{i : x_ik <= v} q_i >= r,
   returned with the bits of the particle that holds it: the inverse CDF
   (type 1).  p = 0 gives the minimum of the support, p = 1 the maximum; the
   result is always the value of a particle with q_i > 0, so for a categorical
   latent it is a class index.  n_probs is 1..16, an interface limit that
   bounds the scratch; n_probs outside it, a NULL probs or out, or a
   probability that is NaN or outside [0, 1]: GH_E_INVAL, before any device
   work.  Otherwise refused as gh_pf_estimate: before init and on the
   multi-rank path GH_E_STATE, t outside 0..T GH_E_INVAL, an earlier step
   without record_history GH_E_STATE, log-weights all -inf (S = 0) or holding
   a NaN or +inf GH_E_NUMERIC.  The filter is only read (t, states, weights,
   log-ML, history, a pending resample and the move counters stay as they are)
   and continues bit for bit.  Every model family. */
int gh_pf_quantiles(gh_pf* pf, int t, int n_probs, const double* probs /* [n_probs] */,
                    double* out /* [n_probs][d] */);
/* Every step's summary in one backward walk of the genealogy: what
   gh_pf_estimate and gh_pf_quantiles return for each step of a range, and per
   step how much of the genealogy still stands behind it.  T calls of
   gh_pf_estimate walk n T (T - 1) / 2 hops per pass and synchronise T times;
   these walk n (T - 1) hops once and synchronise once.
   Range: steps t0..t1 with 1 <= t0 <= t1 <= T, T the current step; t1 = 0
   means T.  L = t1 - t0 + 1 steps; row i of every output is step t0 + i.  A
   range that reaches below T needs record_history.
   Ancestors: a_t(i) is the index, among step t's particles, of the ancestor
   of current particle i, as gh_pf_get_trajectory, gh_pf_estimate and
   gh_pf_quantiles follow it: while a resample is pending first through the
   pending resample's ancestors, then one hop through step s's ancestor array
   for every s in (t, T] that a resample preceded, clamped into [0, n) at
   every hop.
   Integer weights: q_i is gh_pf_quantiles' weight, floor(exp(lw_i - M)
   2^shift), every q_i = 2^shift while a resample is pending; S = sum q_i.  For
   particle j of step t, m_t(j) = sum of q_i over the i with a_t(i) = j, an
   exact unsigned 64-bit sum (S < 2^63).
   Per-step diagnostics:
     distinct[t] = #{ j : m_t(j) > 0 }     the step-t particles that still have a weighted
                                           descendant among the current ones
     ess[t]      = S^2 / sum_j m_t(j)^2    in doubles: the effective sample size of the step-t
                                           marginal the genealogy carries
   The genealogy coalesces going back: distinct is non-decreasing in t,
   ess[t] <= distinct[t], and at t = T without a pending resample distinct is
   the number of particles with q_i > 0.  Where distinct[t] has fallen to a
   handful, mean[t], cov[t] and the quantiles of step t rest on that handful
   of values, whatever n is: the part of a smoothed path with a small
   distinct[t] is not to be trusted.  The sum of squares goes over the
   ancestor slots in a fixed order with no floating-point atomics: two calls
   return the same bits.
   Moments: mean[t] and cov[t] have the bits of gh_pf_estimate(pf, t, ...)'s
   mean and cov (the same weights, the same two-pass algorithm, the same grid
   and the same order of every sum).  Quantiles: out[t][j][k] has the bits of
   gh_pf_quantiles(pf, t, n_probs, probs, ...).
   gh_pf_estimate_path: any of ess, distinct, mean, cov may be NULL; all four
   NULL, or a NULL pf: GH_E_INVAL before any device work.  gh_pf_quantiles_path:
   n_probs outside 1..16, a NULL probs or out, a probability that is NaN or
   outside [0, 1]: GH_E_INVAL before any device work.  Both: before init and
   on the multi-rank path GH_E_STATE; t0 < 1, t1 > T or t0 > t1 GH_E_INVAL;
   t0 < T without record_history GH_E_STATE; d outside 1..16 GH_E_INVAL;
   log-weights all -inf, or holding a NaN or +inf GH_E_NUMERIC.  The filter is
   only read (t, states, weights, log-ML, history, a pending resample and the
   move counters stay as they are) and continues bit for bit.  Scratch of two
   arrays of n words and L result blocks is kept on the filter.  Every model
   family. */
int gh_pf_estimate_path(gh_pf* pf, int t0, int t1, double* ess /* [L] */, int64_t* distinct /* [L] */,
                        double* mean /* [L][d] */, double* cov /* [L][d][d] */);
int gh_pf_quantiles_path(gh_pf* pf, int t0, int t1, int n_probs, const double* probs /* [n_probs] */,
                         double* out /* [L][n_probs][d] */);
/* The posterior predictive of x_{T+k} and y_{T+k}, k = 1..horizon, given the
   data up to the current step T, reduced on the device; the filter is only
   read (t, states, weights, log-ML, history, a pending resample and the move
   counters stay as they are, and it continues bit for bit as a filter that
   made no forecast).  Particle i's latent is advanced by the model's own
   transition with exactly the draws an unobserved default-proposal
   gh_pf_step would use (a custom proposal of the filter is not applied), so
   xs[k-1] holds bit for bit what the filter's states would be after k
   unobserved steps without a resample, under unchanged weights; y_{T+k} is
   drawn from x_{T+k} with gh_simulate's observation noise, keyed by (seed,
   particle, T+k).  Particles and weights are gh_pf_estimate's: the resampled
   particles with equal weights while a resample is pending; a particle of
   weight exactly 0 adds nothing; log-weights all -inf, or holding a NaN or
   +inf: GH_E_NUMERIC.  Per horizon k: the weighted mean and the weighted
   POPULATION covariance (gh_pf_estimate's definitions and two-pass centring,
   exactly symmetric) of x and of y, and optionally the draws themselves in
   gh_simulate's layout.  dy: the model's dy for the LG-SSM and slot models, 1
   for the HMM (the symbol) and Kitagawa.  inputs: [horizon][d], row k-1 the
   input u_{T+k} of a slot model with per-step inputs (latent form 2), which is
   refused without them as every other model is with them; finite values
   only.  Every output may be NULL (all NULL: GH_E_INVAL); the covariances
   cost a second propagation, the draws the only memory of n x horizon.
   horizon is 1..64, an interface limit that bounds the block-partials buffer.
   One rank only (GH_E_STATE on the multi-rank path); not for the regression
   family, which has no time extension (GH_E_INVAL).  One synchronise.
   Deterministic: the same filter gives the same bits. */
int gh_pf_forecast(gh_pf* pf, int horizon, const double* inputs /* [horizon][d] or NULL */,
                   double* x_mean /* [H][d] */, double* x_cov /* [H][d][d] */,
                   double* y_mean /* [H][dy] */, double* y_cov /* [H][dy][dy] */,
                   double* xs /* [H][d][n_local] */, double* ys /* [H][dy][n_local] */);
/* The log-weights as step t left them (1 <= t <= T, T the current step): the
   vector that pairs with the rows of step t's states, before any resample that
   followed.  t = 0 or t = T: the current weights, as gh_pf_get_log_weights
   (zeros while a resample is pending).  An earlier step needs a filter made
   with gh_pf_opts.record_weights (GH_E_STATE otherwise); with it, init and
   every step end in one device-to-device copy of the n log-weights into the
   step's slot, enqueued after everything that writes them (the step kernel,
   a conditional filter's pinning, gh_pf_step_params' re-scoring).  The moves
   (gh_pf_rejuvenate, gh_pf_mh_select, ...) rewrite the step's rows and leave
   its weights alone, so the pairing holds.  With the option off nothing is
   launched, copied or allocated for it.  NULL pf or host_out, t outside 0..T:
   GH_E_INVAL; before init and on the multi-rank path: GH_E_STATE. */
int gh_pf_get_log_weights_at(gh_pf* pf, int t, double* host_out /* n_local */);
/* The backward kernel's log-weights at step t, 1 <= t < T, for a state x_next
   of step t + 1:
     b_i = lw_t[i] + logpdf(x_{t+1} = x_next | x_t = row i of step t)
   one fp64 add of the recorded weight (gh_pf_get_log_weights_at) and the
   latent score of step t + 1, the model's own transition density exactly as
   gh_pf_get_scores evaluates it (per-step inputs and the switching pair
   included): the weights of backward simulation, of the forward-filter
   backward-smoother's marginals, of two-filter smoothing and of ancestor
   sampling.  Unnormalised; -inf where the transition is impossible.  NULL
   argument, t outside 1..T-1, the regression family: GH_E_INVAL; before init,
   on the multi-rank path, without record_weights, or after a
   gh_pf_step_params (the recorded weights were formed under other parameters
   than the density used here): GH_E_STATE. */
int gh_pf_backward_weights(gh_pf* pf, int t, const double* x_next /* [d] */, double* host_out /* [n] */);
/* n_traj draws from the joint smoothing distribution p(x_t0:T | y_1:T) by
   backward simulation (FFBSi: Godsill, Doucet & West 2004) over the filter's
   recorded states and weights.  Unlike the surviving genealogy
   (gh_pf_get_trajectory, gh_pf_estimate_path), whose early steps rest on a
   handful of ancestors, every step of a draw is picked among all n particles
   of that step.  The draws carry equal weight; the filter is only read (t,
   states, weights, log-ML, history, a pending resample and the move counters
   stay as they are) and continues bit for bit.
   Definition (it fixes every bit).  For trajectory m and step t the uniform is
     u = u53(w.x, w.y) 2^53,  w = Philox4x32-10(counter = (m lo, m hi, t, 8 << 16), key = seed)
   the engine's counter layout with stream 8 (STREAM_SMOOTH) and draw 0; u is a
   53-bit integer.  With shift = 62 - ceil(log2 n), at most 52 (the
   resampler's), a vector b of n log-weights gives
     B      = max_i b_i
     q_i    = floor(exp(b_i - B) 2^shift)      an unsigned integer; b_i = -inf: 0
     S      = sum q_i
     target = floor(u S / 2^53)                exact integer arithmetic, < S
     pick   = the first i whose inclusive sum q_0 + ... + q_i exceeds the target
   Start, step T: b = the current log-weights, the pick i* is a current
   particle and j_T = i*; while a resample is pending every q_i = 2^shift and
   j_T = the pending resample's ancestor of i* (the particles and weights of
   gh_pf_quantiles).  Backward, t = T-1 down to t0: b = the backward weights
   (gh_pf_backward_weights) of step t for x_next = row j_{t+1} of step t + 1,
   and j_t = the pick.  Outputs: xs[t - t0][m] = row j_t of step t's states (d
   doubles, with the particle's bits), idx[t - t0][m] = j_t (idx may be NULL).
   Step t's states are the particles as step t (and any move after it) left
   them, the rows gh_pf_get_states returned then, paired with
   gh_pf_get_log_weights_at(pf, t); not gh_pf_get_trajectory(pf, t)'s, which
   are the ancestors of the current particles.
   Integer sums and the fp64 maximum do not depend on their order: the same
   filter, seed and n_traj give the same bits on every run.
   A NaN or +inf among the b_i, or B = -inf (no particle of step t can precede
   the drawn state), at any step of any trajectory: GH_E_NUMERIC, reported
   after the call's one synchronise.  Refused before any device work: NULL pf
   or xs, n_traj outside 1..65536, t0 outside 1..T, the regression family:
   GH_E_INVAL; before init, on the multi-rank path, t0 < T without
   record_weights, a filter that ever stepped through gh_pf_step_params:
   GH_E_STATE.  t0 = T (T = 1 included) is the start draw alone and needs no
   weight history.  Cost: 2 n n_traj transition densities per backward step.
   Scratch kept on the filter until it is destroyed: the block partials (two
   words per 256 particles) of one launch's trajectories, 1024 of them up to
   n = 2^20 and fewer above so that they stay within 64 MiB, but never fewer
   than 64: from n = 2^24 on the scratch is 4.1 n bytes (272 MiB at n = 2^26),
   half of one step's recorded weights; never n x n_traj. */
int gh_pf_smooth(gh_pf* pf, int t0, int64_t n_traj, uint64_t seed, double* xs /* [T-t0+1][n_traj][d] */,
                 int32_t* idx /* [T-t0+1][n_traj] or NULL */);
/* The score columns of the current particles' traces (the per-choice score
   fields of static_ir/trace.jl:91-129): total[i] = get_score(trace i), and
   (nullable) per_step[t-1][0][i] / per_step[t-1][1][i] = the scores of the
   latent :chain => t => :x and the observation :chain => t => :y (0 when not
   observed) — the model's densities, whatever proposal made the particles.
   Computed on the device from the history (record_history, one rank). */
int gh_pf_get_scores(gh_pf* pf, double* total /* [n_local] */, double* per_step /* [t][2][n_local] */);
int gh_pf_sample_unweighted(gh_pf* pf, int64_t n_samples, uint64_t seed, int64_t* host_idx);
/* Rejuvenation: n_moves MH moves on every particle, each regenerating the
   current latent x_t from its prior given x_{t-1} (x_1 from the initial
   distribution) and accepting with log(rand()) < log p(y_t|x'_t) - log p(y_t|x_t).
   Log weights are unchanged.  Call after gh_pf_init / gh_pf_step and before
   gh_pf_maybe_resample (GH_E_STATE otherwise); at most 2^24 moves per step.
   *accepted (optional, synchronises) = accepted moves summed over the local
   particles. */
int gh_pf_rejuvenate(gh_pf* pf, int n_moves, int64_t* accepted);
/* metropolis_hastings(trace, selection) on every particle (src/inference/mh.jl:14-28,
   the selection form): regenerate the selected latent addresses of the current
   step from their prior, accept with log(rand()) < the regenerate weight.
   selection is a bit mask over the step's latent addresses: the Unfold families
   have one (bit 0: :chain => t => :x, the same move as gh_pf_rejuvenate); the
   regression has two (bit 0 :slope, bit 1 :intercept; quickstart.jl:17-22's
   mh(trace, select(:slope)) / mh(trace, select(:intercept))).  The moves share
   gh_pf_rejuvenate's draw windows and per-step move counter. */
int gh_pf_mh_select(gh_pf* pf, uint32_t selection, int n_moves, int64_t* accepted);
/* mh(trace, drift, (sd,)) on every particle (src/inference/mh.jl:41-62, a
   proposal generative function): the Gaussian drift proposal
   `@trace(normal(trace[a], sd), a)` on the selected latent addresses of the
   current step (bit layout as gh_pf_mh_select; the LG-SSM's vector :x drifts
   componentwise with sd[0..d), a diagonal mvnormal), accept iff log(rand()) <
   update weight - fwd score + bwd score (the symmetric drift's two scores
   cancel exactly).  sd[d]: > 0 for the selected components.  Not for the
   HMM (a discrete latent).  Same calling rules and draws as gh_pf_rejuvenate. */
int gh_pf_mh_drift(gh_pf* pf, uint32_t selection, const double* sd /* [d] */, int n_moves, int64_t* accepted);
/* choice_gradients(trace, selection, nothing) on every particle (the GFI's
   choice_gradients, src/gen_fn_interface.jl:374-406; the reference differentiates
   through the trace, src/static_ir/backprop.jl): the values of the current
   step's latent and the gradient of the trace's score with respect to them —
   the step's latent score plus observation score, the current latent having
   no children yet.  The gradients are closed forms of the hand-lowered
   continuous families (LG-SSM, nonlinear SSM, regression; gh_grad.h); the HMM
   and slot-described models are not lowered (GH_E_INVAL).  selection: bit
   layout as gh_pf_mh_select; unselected components of the regression get
   gradient 0.  host_values (optional) and host_grads are [d][n_local].  One
   rank, not a conditional filter, after a step and before
   gh_pf_maybe_resample (GH_E_STATE otherwise); the regression at t = 1. */
int gh_pf_choice_gradients(gh_pf* pf, uint32_t selection, double* host_values /* [d][n_local], nullable */,
                           double* host_grads /* [d][n_local] */);
/* mala(trace, selection, tau) on every particle (src/inference/mala.jl:11-54):
   propose normal(x + tau grad(x), sqrt(2 tau)) on the selected components of
   the current latent, accept iff log(rand()) < update weight - fwd score +
   bwd score.  tau finite and > 0.  Families, calling rules and refusals as
   gh_pf_choice_gradients; draw windows and the per-step move counter are
   shared with gh_pf_rejuvenate (at most 2^24 moves per step).  Log weights
   are unchanged.  *accepted (optional, synchronises) as gh_pf_rejuvenate. */
int gh_pf_mala(gh_pf* pf, uint32_t selection, double tau, int n_moves, int64_t* accepted);
/* hmc(trace, selection; L, eps) on every particle (src/inference/hmc.jl:25-72):
   standard normal momenta on the selected components, L >= 1 leapfrog steps
   of size eps (finite, > 0), accept iff log(rand()) < new score - old score +
   new kinetic - old kinetic.  Otherwise as gh_pf_mala. */
int gh_pf_hmc(gh_pf* pf, uint32_t selection, int L, double eps, int n_moves, int64_t* accepted);
/* elliptical_slice(trace, addr, mu, cov) on every particle
   (src/inference/elliptical_slice.jl:13-45; Murray, Adams, MacKay 2010): the
   selected latent address of the current step moves on the ellipse through
   its value and a fresh draw nu ~ N(0, cov), the angle shrinking towards the
   current value until the slice test passes.  mu and cov are the model's own
   prior of the address given the particle's parent, hence no arguments.  The
   slice is on the likelihood alone: accept iff loglik(x') - loglik(x) > log u.
   The reference compares the whole update weight, which counts the prior of
   the moved address twice and leaves prior^2 x likelihood invariant; that
   arithmetic is deliberately not reproduced.  No step size, no rejection; a
   move is capped at 64 shrinks, after which the particle stays where it is
   and counts in *exhausted.  selection: one address (the regression: :slope
   or :intercept, not both: GH_E_INVAL).  Families, calling rules and refusals
   as gh_pf_choice_gradients; draw windows and the per-step move counter are
   shared with gh_pf_rejuvenate.  Log weights are unchanged.  *shrinks (total
   over particles and moves) and *exhausted are optional and synchronise. */
int gh_pf_elliptical_slice(gh_pf* pf, uint32_t selection, int n_moves, int64_t* shrinks /* nullable */,
                           int64_t* exhausted /* nullable */);
/* map_optimize(trace, selection; max_step_size, tau, min_step_size) on every
   particle, n_iters times (src/inference/map_optimize.jl:9-41): backtracking
   gradient ascent on the step's score over the selected components of the
   current latent — try x + step grad(x) from step = max_step_size, multiply
   step by tau while the score got worse, give up (keep x) once step <
   min_step_size.  max_step_size and min_step_size finite and > 0, tau in
   (0, 1), and at most 1100 backtracking steps from max to min (GH_E_INVAL
   otherwise).  Draws nothing: the per-step move counter does not advance.
   Families, calling rules and refusals as gh_pf_choice_gradients.  Log
   weights are unchanged.  *improved (optional, synchronises): iterations that
   moved, over this rank's particles. */
int gh_pf_map_optimize(gh_pf* pf, uint32_t selection, double max_step_size, double tau, double min_step_size,
                       int n_iters, int64_t* improved /* nullable */);
/* Conditional SMC (examples/pmmh/smc.jl:100-151, the particle-Gibbs sweep):
   particle 0 is the distinguished particle, pinned to ref_x1 at init and to
   ref_xt at each step, its parent always itself, its weight the observation
   log-density of the given state (init_score / forward_score of the model's
   own proposal).  Requires opts->resampler == GH_RESAMPLE_MULTINOMIAL and one
   rank.  Such a filter steps only with gh_pf_step_conditional.
   Ancestor sampling (opts->ancestor_sampling = 1; particle Gibbs with ancestor
   sampling, PGAS: Lindsten, Jordan & Schon, JMLR 2014).  smc.jl:136-139 make the
   distinguished particle its own parent at every step, so a new reference
   shares its early steps with the old one unless n grows with T.  With the
   option, at a step t >= 2 whose resample fired (a gh_pf_maybe_resample since
   step t - 1 that decided to resample) gh_pf_step_conditional draws that
   parent among all n particles of step t - 1 with probability proportional to
   exp(b_i),
     b_i = lw_{t-1}[i] + logpdf(x_t = ref_xt | x_{t-1} = row i of step t - 1)
   the bits of gh_pf_backward_weights(pf, t - 1, ref_xt) on a filter that also
   records its weights (the option itself does not need record_weights): the
   log-weights as step t - 1 left them, which a pending resample does not
   rewrite, plus the model's own transition density, one fp64 add.  The
   selection is gh_pf_smooth's integer rule unchanged (B, q_i, S, target and
   the first inclusive sum that exceeds it) under the uniform
     u = u53(w.x, w.y) 2^53,  w = Philox4x32-10(counter = (0, 0, t, 10 << 16), key = the filter's seed)
   stream 10 (STREAM_ANCESTOR), draw 0.  The pick J replaces the 0 in entry 0
   of the ancestors step t consumes, in stream order after the resample's own
   writes, so gh_pf_get_parents shows it once the step has run.  Nothing else
   changes: particle 0's state and weight are ref_xt and the observation
   log-density, every other particle's parent, state and weight have the bits
   they have without the option, and gh_pf_get_trajectory, gh_pf_get_scores,
   the *_path walks and the recorded history follow the new parent through
   the genealogy they already read.  Where no resample fired the ancestors are
   not read and particle 0 continues itself as without the option: its parent
   is then no random variable, which keeps the sweep a valid conditional SMC
   under an adaptive ESS threshold.  No host synchronisation is added to the
   step; three launches that read each row of step t - 1 once; scratch of
   8 n + n / 16 bytes allocated by gh_pf_init_conditional.  With the option
   off nothing is launched or allocated.
   A NaN or +inf among the b_i, or B = -inf (no particle can precede ref_xt),
   raises GH_E_NUMERIC on the device: it is returned by the next call that
   reads the device status (gh_pf_maybe_resample with an output,
   gh_pf_log_ml_estimate, ...).  Refused before any device work: the option on
   gh_pf_init / gh_pf_init_q: GH_E_INVAL; on a multi-rank context: GH_E_STATE;
   gh_pf_step_params_conditional on a filter with the option: GH_E_STATE (the
   weights of step t - 1 would have to be the re-scored ones). */
int gh_pf_init_conditional(gh_model* m, const gh_obs* obs, int64_t n_particles, uint64_t seed,
                           const gh_pf_opts* opts, const double* ref_x1 /* [d] */, gh_pf** out);
int gh_pf_step_conditional(gh_pf* pf, const gh_obs* obs, const double* ref_xt /* [d] */);
/* per-step resampling record: ess and did_resample for steps 1..t */
int gh_pf_get_ess_history(gh_pf* pf, int max_steps, double* ess, int32_t* did);
/* average duration (ms) of the step kernel over the timed launches (opts.time_kernels) */
int gh_pf_kernel_time(gh_pf* pf, double* avg_ms, int64_t* n_launches, int reset);

/* multi-rank systematic resampling plan (host only, no GPU): given every
   rank's integer weight total and the shared offset o < sum(totals), the global
   slot ranges rank `rank` sends to ([send_lo[r], send_hi[r])) and receives from
   ([recv_lo[r], recv_hi[r])) each rank r; empty ranges have lo == hi.  This is
   the plan gh_pf_maybe_resample follows; exposed for tests and integrators. */
int gh_sys_plan(int64_t n_global, int world, int rank, const uint64_t* totals, uint64_t offset,
                int64_t* send_lo, int64_t* send_hi, int64_t* recv_lo, int64_t* recv_hi);
/* the grouped messages that plan becomes (host only): peers and byte counts of
   the sends and receives, rows of d + 1 doubles, in the order both transports
   post them (RCCL ncclSend/ncclRecv in one group, or gh_host_comm.sendrecv).
   Arrays hold up to world - 1 entries. */
int gh_debug_exchange_lists(int64_t n_global, int world, int rank, const uint64_t* totals, uint64_t offset, int d,
                            int* n_send, int* send_peer, uint64_t* send_bytes, int* n_recv, int* recv_peer,
                            uint64_t* recv_bytes);

/* test hook: widen the ancestor field of the filter's 32-bit range marks to
   `bits` (at least what the particle count needs, at most 31), which shortens
   the epoch field, so that a short run crosses several epoch wraps (the marks
   are cleared at each).  Only before the first resample is pending. */
int gh_debug_mark_bits(gh_pf* pf, int bits);

/* test hook: overwrite the genealogy record of step t (2 <= t <= current):
   particle j's ancestor index becomes `value` (a corrupted record, so that a
   test can check that a genealogy query reports GH_E_STATE instead of
   returning a wrong trajectory).  The filter is unusable afterwards. */
int gh_debug_set_ancestor(gh_pf* pf, int t, int64_t j, int32_t value);

/* test hook: the systematic slot counts are taken in floating point and
   recounted exactly when within a window of an integer (2^(ceil(log2 N) + 7 - 53)
   by default, so rarely); log2_inv > 0 sets the window to 2^-log2_inv for every
   later resample on the context's device, so that the exact recount runs often
   (0 restores the default).  Results do not change. */
int gh_debug_count_window(gh_ctx* ctx, int log2_inv);

/* ---- importance sampling ---------------------------------------------------- */
int gh_is_run(gh_model* m, const gh_obs* obs, int proposal, int64_t n, uint64_t seed,
              double* host_log_norm_weights /* may be NULL */, double* host_states /* may be NULL */,
              double* lml);

/* ---- particle-marginal MH (config C5) ------------------------------------------
   examples/pmmh/example.jl:20-79: log var_x, log var_y ~ normal(0, 2); the
   likelihood is the log-ML estimate of an inner particle filter with n_inner
   particles on the Kitagawa model (examples/pmmh/pf.jl:14-73); each
   iteration applies mh(select(:var_x)), mh(select(:var_y)) and the two
   random-walk moves (sd sqrt(0.5)) (src/inference/mh.jl:14-62).  One
   workgroup per chain, chains [chain0, chain0 + n_chains) (a rank's share).
   init = 1 draws the start from the prior (generate); otherwise lvx / lvy /
   lml hold the state to continue from, after iter0 iterations.  Host buffers; hist (nullable) gets
   [n_chains][n_iters][2]; accepts [n_chains][4] counts per move. */
int gh_pmmh_run(gh_ctx* ctx, int64_t chain0, int64_t n_chains, int n_inner, const double* ys, int T,
                int n_iters, int iter0, uint64_t seed, int init, double* lvx, double* lvy, double* lml, int32_t* accepts,
                double* hist, double* kernel_ms);

/* ---- reversible-jump MH on the coal change-point model (config C3) ---------------
   examples/coal/coal.jl:47-62 model, mcmc_step (:329-336) = rate_move,
   position_move (k > 0), birth_death_move, each an involutive MH step
   (src/inference/mh.jl:85-98, trace_translators.jl:848-876).  One thread per
   chain; events sorted, T = events[E-1].  state: host [n_chains][68] rows
   (k, score, cp[32], h[33], pad), written on return and read when init == 0
   (continuing after iter0 iterations).  accepts [n_chains][3]; khist
   (nullable) [n_chains][n_iters] = k after each iteration. */
int gh_coal_run(gh_ctx* ctx, int64_t chain0, int64_t n_chains, const double* events, int E, int n_iters,
                int iter0, uint64_t seed, int init, double* state, int32_t* accepts, int32_t* khist,
                double* kernel_ms);

/* Device-resident chains (the same kernel, state kept in HBM between calls:
   no per-call state upload/download).  gh_coal_step's first call draws the
   start from the prior (generate) and then runs n_iters iterations; later
   calls continue.  accepts (nullable) [n_chains][3]: this call's counts;
   khist as gh_coal_run.  gh_coal_read_state: the [n_chains][68] rows. */
typedef struct gh_coal gh_coal;
int gh_coal_create(gh_ctx* ctx, int64_t chain0, int64_t n_chains, const double* events, int E, uint64_t seed,
                   gh_coal** out);
int gh_coal_step(gh_coal* h, int n_iters, int32_t* accepts, int32_t* khist, double* kernel_ms);
/* the MCMC kernel of the following gh_coal_step calls: 0 = mcmc_step (rate,
   position, birth/death; coal.jl:329-336, the default), 1 = simple_mcmc_step
   (rate, position, then mh(trace, select(:k)) — the Dynamic DSL regenerate of
   k with the change points and rates it adds or drops; coal.jl:338-345);
   accepts[2] counts the third move's acceptances either way */
int gh_coal_set_kernel(gh_coal* h, int kernel);
int gh_coal_read_state(gh_coal* h, double* state);
/* Resume the chains from given rows ([n_chains][68], the layout of
   gh_coal_read_state: fields past k / k+1 zero); the next gh_coal_step
   continues at iteration iter0 + 1 (its draws are those of that iteration). */
int gh_coal_write_state(gh_coal* h, const double* state, int iter0);
int gh_coal_destroy(gh_coal* h);

/* ---- diagnostics ------------------------------------------------------------ */
const char* gh_last_error(void);
const char* gh_version(void);
/* device self-test: evaluates gh_exp/gh_log/sqrt/div/normals on n inputs on the
   GPU so tests can compare them bit-for-bit with the CPU oracle (out_div: the
   even entries in[i] / in[i+1], the odd ones the models' in[i] / 20) */
int gh_selftest_math(gh_ctx* ctx, int64_t n, const double* in, double* out_exp, double* out_log,
                     double* out_sqrt, double* out_div);
/* Box–Muller stages for n word triples (a, b, c): out[4i..4i+3] =
   (1 - u53(a, b), sqrt(-2 log(.)), z0, z1) as the kernels compute them */
int gh_selftest_boxmuller(gh_ctx* ctx, int64_t n, const uint32_t* words, double* out);
int gh_selftest_normals(gh_ctx* ctx, uint64_t seed, int64_t n, uint32_t step, uint32_t stream,
                        int dim, double* out /* [n][dim] */);

#ifdef __cplusplus
}
#endif
#endif
