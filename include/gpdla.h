/* gpdla.h -- C-ABI of the MI355X-native GP/DLA inference sweep (libgpdla.so).
 *
 * Drop-in boundary for ONE hot path of jibanCat/gp_dla_detection: the per-spectrum GP
 * marginal-likelihood sweep.  The reference has no plugin registry; the path sits behind three
 * plain call surfaces, and each entry point below replaces one of them (paths relative to the
 * reference tree):
 *
 *   gpdla_voigt                  <-  voigt.c:253-304          MEX gateway  voigt(lambdas, z, N[, num_lines])
 *   gpdla_log_mvnpdf_low_rank    <-  log_mvnpdf_low_rank.m:5  log_p = log_mvnpdf_low_rank(y, mu, M, d)
 *   gpdla_process_batch          <-  process_qsos.m:88-233    the per-quasar loop + posteriors
 *   gpdla_process_batch_multi    <-  multi_dlas/process_qsos_multiple_dlas_meanflux.m:141-495
 *
 * plus a resident-data form (context + uploaded batch) so that a caller that keeps spectra in HBM
 * -- the production case, and what bench.py times -- pays no PCIe inside the sweep.
 *
 * Conventions: plain pointers and sizes only, caller owns every buffer,
 * no global state, all arithmetic IEEE fp64, MATLAB matrices are column-major, every function
 * returns 0 or a negative gpdla_status.  All compute runs in hand-written HIP kernels for gfx950;
 * there is NO CPU fallback: without a usable GPU every compute entry point returns
 * GPDLA_ERR_NO_DEVICE.
 */
#ifndef GPDLA_H
#define GPDLA_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  GPDLA_OK = 0,
  GPDLA_ERR_INVALID_ARGUMENT = -1, /* null pointer, n_padded <= 6, num_lines outside [1,31], ... */
  GPDLA_ERR_NO_DEVICE = -2,        /* no HIP device / device_id out of range */
  GPDLA_ERR_HIP = -3,              /* a HIP runtime call failed; see gpdla_last_error() */
  GPDLA_ERR_NOT_POSITIVE_DEFINITE = -4, /* chol(B) would throw, log_mvnpdf_low_rank.m:24 */
  GPDLA_ERR_UNSUPPORTED = -5,      /* e.g. k > GPDLA_MAX_K */
  GPDLA_ERR_HOST = -6              /* host side: out of memory, a stage thread could not be started, or an
                                      unexpected C++ exception -- none ever crosses this boundary */
} gpdla_status;

#define GPDLA_MAX_K 40
#define GPDLA_ABI_VERSION 6

int gpdla_abi_version(void);
/* Human-readable text of the most recent error on this thread (never NULL). */
const char *gpdla_last_error(void);

/* ---------------------------------------------------------------------------------------------
 * Stateless single-call surfaces (host pointers; device chosen by device_id).
 * ------------------------------------------------------------------------------------------- */

/* voigt.c:253-304.  profile_out has n_padded - 6 entries (numel(lambdas) - 2*width, :271).
 * num_lines in [1, 31] (the MEX default when the 4th argument is omitted is 31, :16, :266).
 * The reference validates nothing; here bad arguments return GPDLA_ERR_INVALID_ARGUMENT. */
int gpdla_voigt(const double *lambdas, int64_t n_padded, double z, double N, int num_lines,
                double *profile_out, int device_id);

/* log_mvnpdf_low_rank.m:5-34.  y, mu, d: n;  M: n x k column-major (ld = n).  A non-PD
 * B = I + M' D^-1 M returns GPDLA_ERR_NOT_POSITIVE_DEFINITE and *log_p = NaN (MATLAB: chol throws).
 * The MATLAB function takes any k; this stand-alone surface accepts k <= 256 (the batch sweep,
 * whose accumulators live in registers, is the one limited to GPDLA_MAX_K). */
int gpdla_log_mvnpdf_low_rank(const double *y, const double *mu, const double *M, const double *d,
                              int64_t n, int k, double *log_p, int device_id);

/* ---------------------------------------------------------------------------------------------
 * Batch surface: process_qsos.m.
 * ------------------------------------------------------------------------------------------- */

/* learned_qso_model_*.mat, process_qsos.m:30-35 (written by learn_qso_model.m:113-123). */
typedef struct {
  int32_t num_rest_pixels;          /* G = numel(rest_wavelengths) */
  int32_t k;                        /* columns of M (set_parameters.m:36) */
  const double *rest_wavelengths;   /* [G] ascending */
  const double *mu;                 /* [G] */
  const double *M;                  /* [G x k] column-major */
  const double *log_omega;          /* [G] */
  double log_c_0, log_tau_0, log_beta;
} gpdla_model;

/* dla_samples.mat, process_qsos.m:38-40 (+ lls_nhi_samples of set_lls_parameters.m:59-63 for the
 * multi-DLA driver; may be NULL otherwise). */
typedef struct {
  int64_t num_dla_samples;          /* S (set_parameters.m:48) */
  const double *offset_samples;     /* [S] in [0,1) */
  const double *log_nhi_samples;    /* [S]  (only the multi-DLA MAP bookkeeping reads it) */
  const double *nhi_samples;        /* [S] */
  const double *lls_nhi_samples;    /* [S] or NULL */
} gpdla_samples;

/* preloaded_qsos.mat's ragged cell arrays (preload_qsos.m:64-79) flattened CSR-style, after the
 * test_ind subset of process_qsos.m:56-61, plus the per-quasar scalars the loop reads. */
typedef struct {
  int64_t num_quasars;
  const int64_t *offsets;           /* [num_quasars + 1] into the four pixel arrays */
  const double *wavelengths;        /* observed, Angstrom */
  const double *flux;
  const double *noise_variance;     /* of a kept pixel: > 0 (else status 3).  +inf gives -inf
                                       log-likelihoods, as in the reference; a finite nu above 1e100
                                       adds -log(nu)/2 outside the sweep, dropping terms below 1e-39 */
  const uint8_t *pixel_mask;        /* nonzero = masked */
  const double *z_qsos;             /* [num_quasars] */
  const double *log_priors_no_dla;  /* [num_quasars]  process_qsos.m:130-131 (host logic) */
  const double *log_priors_dla;     /* [num_quasars]  process_qsos.m:128-129; multi: [nq][max_dlas] (multi :204) */
  const double *log_priors_lls;     /* multi only (:208-210), else NULL */
} gpdla_spectra;

/* The set_parameters.m values the loop reads (process_qsos.m:104-105, 118, 159-176, 188). */
typedef struct {
  double min_lambda, max_lambda;    /* set_parameters.m:33-34 */
  double lya_wavelength;            /* :5  */
  double lyman_limit;               /* :7  */
  double pixel_spacing;             /* :60 */
  double max_z_cut, min_z_cut;      /* :65, :69 */
  int32_t width;                    /* :59 -- must be 3 (voigt.c:229 hard-codes it) */
  int32_t num_lines;                /* :63 */
  /* multi-DLA only (process_qsos_multiple_dlas_meanflux.m:32-37, set_parameters_multi.m:75) */
  int32_t max_dlas;
  int32_t num_forest_lines;
  double min_z_separation;
  double prev_tau_0, prev_beta;
  /* weighted resampling of the multi-DLA driver when base_sample_inds is not supplied: the draw
   * for (quasar, model, index) depends only on rng_seed and first_quasar_index + local quasar
   * index, so shards of one run pass their global offset here and agree with an unsharded run */
  uint64_t rng_seed;
  int64_t first_quasar_index;
  /* 0 (default): the [W|U]*[P|M] contraction in fp64 (parity-grade).  1: BASELINE config 5's study
   * variant -- contraction on the fp32 matrix cores, everything else (Voigt profile, weights,
   * quadratic form, log-determinant, Cholesky) in fp64.  Not parity-grade; single-DLA sweep only. */
  int32_t contraction_precision;
  /* multi-DLA driver: bytes of HBM the per-quasar Voigt profile table (2 S rows per quasar) may take
   * at a time; quasars are swept in sub-batches that fit.  0 = default (16 GiB).  The table is
   * scratch of one gpdla_batch_process_multi call and belongs to the CONTEXT: it is allocated on
   * first use, grows only, is shared by all batches of the context and freed with it (the calls of
   * one context are serialized on its stream; two threads' calls take turns). */
  int64_t multi_profile_bytes;
  /* single-DLA sweep: bytes of HBM the per-K-step records of a batch may take at a time.  A batch
   * whose records exceed it is swept in groups of quasars (records built, then swept, group after
   * group into the same pool), so that the resident size of a batch is its spectra and results, not
   * its records: 0.9 KB per K-step for k <= 20, but 29 KB for 20 < k <= 40 -- 228 GB for a DR12Q
   * shard.  Results do not depend on it.  0 = default (16 GiB). */
  int64_t record_pool_bytes;
  /* one-shot entries (gpdla_process_batch, gpdla_process_batch_multi) only: the quasars of a call are
   * swept in HBM-resident batches of at most max_quasars_per_batch through pipeline_slots batch slots
   * (upload of batch i+1 / sweep of batch i / download of batch i-1 overlap).  0 = defaults: 3 slots,
   * gpdla_default_batch_quasars() quasars.  Results do not depend on either. */
  int32_t pipeline_slots;
  int64_t max_quasars_per_batch;
} gpdla_config;

/* Fills a gpdla_config with the reference's defaults (set_parameters.m / set_parameters_multi.m). */
void gpdla_default_config(gpdla_config *cfg);

/* Outputs of process_qsos.m:74-82, 224-233 (field names of :236-244).  Caller-owned; any pointer
 * may be NULL to skip that field.  Entries of spectra that cannot be processed (no pixel survives
 * the selection) are set to NaN, exactly as the reference's NaN pre-fill leaves them.
 * sample_log_likelihoods_dla is [num_quasars][S] with the quasar index slowest (element
 * (quasar_ind, i) of the MATLAB array at [quasar_ind * S + i]). */
typedef struct {
  double *min_z_dlas;                 /* [nq] */
  double *max_z_dlas;                 /* [nq] */
  double *log_likelihoods_no_dla;     /* [nq] */
  double *sample_log_likelihoods_dla; /* [nq][S] */
  double *log_likelihoods_dla;        /* [nq] */
  double *log_posteriors_no_dla;      /* [nq] */
  double *log_posteriors_dla;         /* [nq] */
  double *model_posteriors;           /* [nq][2] = (no DLA, DLA) */
  double *p_no_dlas;                  /* [nq] */
  double *p_dlas;                     /* [nq] */
  int32_t *status;                    /* [nq] 0 ok, 1 = empty spectrum (multi: all_exceptions, :232),
                                         3 = a kept pixel with noise variance <= 0 or NaN (skipped; any
                                         other variance, huge or +inf, is computed as the reference does) */
  /* generate_ascii_catalog.m:73-80, found by the evidence kernel while it walks the table anyway:
   * [~, map_ind] = nanmax(sample_log_likelihoods_dla(i, :)) (1-based, first index on ties; 1 for an
   * all-NaN row, as MATLAB returns), map_z_dla = min_z + (max_z - min_z) * offset_samples(map_ind),
   * log_nhi_samples(map_ind) (log10 of nhi_samples(map_ind) when log_nhi_samples was not given). */
  double *MAP_inds;                   /* [nq] */
  double *MAP_z_dlas;                 /* [nq] */
  double *MAP_log_nhis;               /* [nq] */
} gpdla_results;

/* One-shot: host buffers in, host buffers out -- the loop of process_qsos.m:88 over ALL quasars of the
 * call.  Inside, the quasars are cut into blocks (config->max_quasars_per_batch) that go through
 * config->pipeline_slots batch slots in HBM: one library thread uploads block i+1 (the CSR arrays are
 * sliced in place, nothing is copied on the host) and another downloads block i-1 straight into the
 * caller's arrays while the calling thread has block i swept, so the PCIe copies hide behind the
 * sweeps (INTEGRATION.md section 3 states the measured rate against the resident form).  Host memory
 * beyond the caller's arrays: per-quasar bookkeeping of `slots` blocks.  The call owns a context for
 * its duration (streams, model, samples, slots) and returns when every result is in the caller's
 * arrays; on an error no result array is meaningful.  Results are bit-identical for every batching. */
int gpdla_process_batch(const gpdla_model *model, const gpdla_samples *samples,
                        const gpdla_spectra *spectra, const gpdla_config *config,
                        gpdla_results *results, int device_id);

/* The same loop with the spectra as preloaded_qsos.mat holds them (preload_qsos.m:64-79): ONE ARRAY PER
 * QUASAR -- the cells of all_wavelengths / all_flux / all_noise_variance / all_pixel_mask (after the
 * test_ind subset of process_qsos.m:56-61), or a Python list of NumPy arrays.  Nothing is flattened
 * up front: the library's upload thread copies block i+1 of the cells into the staging vectors of
 * its batch slot while block i is swept, so the host copy hides behind the sweeps like the PCIe
 * copies do (host memory beyond the caller's arrays: `slots` blocks of spectra).  pixel_mask cells
 * are one byte per pixel, nonzero = masked (mxLogical and numpy.bool_ as they are). */
typedef struct {
  int64_t num_quasars;
  const int64_t *num_pixels;              /* [nq] entries of each of the four cells of quasar q */
  const double *const *wavelengths;       /* [nq] pointers */
  const double *const *flux;
  const double *const *noise_variance;
  const uint8_t *const *pixel_mask;
  const double *z_qsos;                   /* [nq] */
  const double *log_priors_no_dla;        /* [nq] */
  const double *log_priors_dla;           /* [nq]; multi: [nq][max_dlas] */
  const double *log_priors_lls;           /* multi only, else NULL */
} gpdla_spectra_cells;
int gpdla_process_cells(const gpdla_model *model, const gpdla_samples *samples,
                        const gpdla_spectra_cells *spectra, const gpdla_config *config,
                        gpdla_results *results, int device_id);

/* Quasars per batch the one-shot entries (and the Python file pipeline) use by default: small enough
 * that `slots` batches of quasars of `longest_spectrum` pixels fit budget_bytes of HBM (0 = 96 GiB)
 * next to the record pool, and that a run has ~8 batches to overlap, at least 128 so that a launch
 * fills the 256 CUs many times over, at most 4096.  multi_models = max_dlas + 1 for the multi-DLA
 * driver (its batches also hold 2 x models sample tables and all their records), else 0.  No GPU. */
int64_t gpdla_default_batch_quasars(int64_t num_quasars, int64_t longest_spectrum, int k,
                                    int64_t num_dla_samples, int slots, int64_t budget_bytes,
                                    int multi_models);

/* ---------------------------------------------------------------------------------------------
 * Resident form: a context owns a device, a stream, the replicated model + samples and scratch;
 * a batch owns spectra in HBM.  Nothing here synchronises the device except where stated.
 * ------------------------------------------------------------------------------------------- */
typedef struct gpdla_context gpdla_context;
typedef struct gpdla_batch gpdla_batch;

int gpdla_context_create(int device_id, gpdla_context **ctx);
void gpdla_context_destroy(gpdla_context *ctx);
/* Use the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) for all launches;
 * NULL restores the context's own stream. */
int gpdla_context_set_stream(gpdla_context *ctx, void *hip_stream);
int gpdla_context_set_model(gpdla_context *ctx, const gpdla_model *model);      /* H2D copy */
int gpdla_context_set_samples(gpdla_context *ctx, const gpdla_samples *samples);/* H2D copy */
int gpdla_context_set_config(gpdla_context *ctx, const gpdla_config *config);
/* Sets config.first_quasar_index alone.  gpdla_context_set_config replaces the whole configuration and
 * must not run while another thread uploads or re-fills a batch of this context (the upload reads
 * the configuration); this call touches one field no upload reads, so the thread that launches the
 * sweeps of a host pipeline may call it per batch while its upload thread is busy (the value is
 * read by the next gpdla_batch_process_multi on the calling thread). */
int gpdla_context_set_first_quasar_index(gpdla_context *ctx, int64_t first_quasar_index);
int gpdla_context_synchronize(gpdla_context *ctx);

/* Copies a CSR batch of spectra to HBM and allocates its result table there.  With
 * spectra->log_priors_lls != NULL the batch is a multi-DLA batch: log_priors_dla is then
 * [nq][max_dlas] (max_dlas of the context's config at this call) and the batch is processed with
 * gpdla_batch_process_multi. */
int gpdla_batch_upload(gpdla_context *ctx, const gpdla_spectra *spectra, gpdla_batch **batch);
/* Re-fills an existing batch with another set of spectra (any size, same or other kind), reusing
 * its device allocations where they are large enough: the batch slots of a host pipeline -- the
 * loop process_qsos.m:88 runs serially -- do no allocation in the steady state.  The batch's
 * previous results must have been downloaded (or be no longer wanted). */
int gpdla_batch_reload(gpdla_context *ctx, gpdla_batch *batch, const gpdla_spectra *spectra);
/* Safe in either order with gpdla_context_destroy (a batch whose context went first only frees
 * its memory). */
void gpdla_batch_destroy(gpdla_batch *batch);

/* The hot path: selection + interpolation (process_qsos.m:102-146), null evidence (:149-151),
 * S-sample Voigt/low-rank sweep (:185-199), evidence + posteriors (:203-213, :224-233) for every
 * quasar of the batch.  Asynchronous on the context's stream; results stay in HBM. */
int gpdla_batch_process(gpdla_context *ctx, gpdla_batch *batch);

/* D2H copy of the batch's results; returns when they are in the caller's arrays.  Uploads,
 * reloads and downloads run on the context's own copy streams, ordered against the batch's own
 * sweep by events: they do not wait for a sweep of ANOTHER batch in flight on the compute stream,
 * so a host pipeline can upload batch i+1 and download batch i-1 while batch i is swept.  The
 * entry points of one context may be called from several threads as long as each batch is used
 * by one thread at a time. */
int gpdla_batch_download(gpdla_context *ctx, gpdla_batch *batch, gpdla_results *results);

/* Device pointer to the per-quasar summary table of the batch, [nq][GPDLA_SUMMARY_COLS] doubles:
 * min_z_dla, max_z_dla, log_prior_no_dla, log_prior_dla, log_likelihood_no_dla, log_likelihood_dla,
 * log_posterior_no_dla, log_posterior_dla, model_posterior[0], model_posterior[1], p_no_dla, p_dla,
 * MAP_ind (1-based), MAP_z_dla, MAP_log_nhi (generate_ascii_catalog.m:73-80).
 * This is the row a multi-GPU run all-gathers. */
#define GPDLA_SUMMARY_COLS 15
int gpdla_batch_summary_device_ptr(gpdla_batch *batch, double **table, int64_t *num_quasars);
/* Device pointer to sample_log_likelihoods_dla [nq][S] of the batch. */
int gpdla_batch_samples_device_ptr(gpdla_batch *batch, double **table, int64_t *num_quasars,
                                   int64_t *num_samples);

/* Profiling aid for bench.py: duration in ms of the most recent sweep-kernel launch of this
 * context, measured with hipEvents on the launch stream (synchronises).  Negative if none. */
double gpdla_context_last_sweep_ms(gpdla_context *ctx);
/* Enables/disables the hipEvent bracketing above (off by default: zero overhead). */
int gpdla_context_set_timing(gpdla_context *ctx, int enabled);

/* ---------------------------------------------------------------------------------------------
 * Multi-DLA driver: multi_dlas/process_qsos_multiple_dlas_meanflux.m.
 * base_sample_inds: [nq][max_dlas-1][S] uint32, 1-BASED as in the reference's output file (:116,
 * :476).  MATLAB's rng('default') + randsample stream (:143, :471-472) cannot be reproduced outside
 * MATLAB, so either the caller supplies the indices (replaying a
 * reference output, or for parity tests), or passes NULL and they are drawn on the GPU with a
 * documented counter-based generator (Philox4x32-10, inverse-CDF sampling; config->rng_seed).
 * Either way the indices used are returned in results->base_sample_inds.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  double *min_z_dlas, *max_z_dlas;        /* [nq] */
  double *log_likelihoods_no_dla;         /* [nq] */
  double *sample_log_likelihoods_dla;     /* [nq][max_dlas][S] */
  double *sample_log_likelihoods_lls;     /* [nq][S] */
  double *log_likelihoods_dla;            /* [nq][max_dlas] */
  double *log_likelihoods_lls;            /* [nq] */
  double *log_posteriors_no_dla;          /* [nq] */
  double *log_posteriors_lls;             /* [nq] */
  double *log_posteriors_dla;             /* [nq][max_dlas] */
  double *model_posteriors;               /* [nq][2 + max_dlas] = (no DLA, LLS, 1..max_dlas DLAs) */
  double *p_no_dlas, *p_lls, *p_dlas;     /* [nq] */
  double *MAP_z_dlas, *MAP_log_nhis, *MAP_inds; /* [nq][max_dlas(model)][max_dlas(slot)], NaN unused */
  uint32_t *base_sample_inds;             /* [nq][max_dlas-1][S], 1-based: the indices used (:476) */
  int32_t *status;                        /* [nq] 1 = all_exceptions (:232) */
} gpdla_results_multi;

/* One-shot form, pipelined like gpdla_process_batch (blocks of quasars through batch slots; block b's
 * draws are keyed by config->first_quasar_index + its first quasar, so the batching does not change
 * them). */
int gpdla_process_batch_multi(const gpdla_model *model, const gpdla_samples *samples,
                              const gpdla_spectra *spectra, const uint32_t *base_sample_inds,
                              const gpdla_config *config, gpdla_results_multi *results,
                              int device_id);

/* ... and with one array per quasar (gpdla_spectra_cells, see gpdla_process_cells). */
int gpdla_process_cells_multi(const gpdla_model *model, const gpdla_samples *samples,
                              const gpdla_spectra_cells *spectra, const uint32_t *base_sample_inds,
                              const gpdla_config *config, gpdla_results_multi *results,
                              int device_id);

/* Resident form of the same driver: the batch was uploaded with log_priors_lls (see
 * gpdla_batch_upload).  base_sample_inds: HOST pointer [nq][max_dlas-1][S] (1-based; an entry 0
 * means "never drawn", as in the rows the reference leaves zero after its early exit, :116,
 * :460-464 -- a sample that would consume it gets NaN; entries > S are rejected) or NULL to draw
 * on the GPU.  Asynchronous on the context's stream apart from that one H2D copy; every result
 * stays in HBM until gpdla_batch_download_multi. */
int gpdla_batch_process_multi(gpdla_context *ctx, gpdla_batch *batch,
                              const uint32_t *base_sample_inds);
int gpdla_batch_download_multi(gpdla_context *ctx, gpdla_batch *batch, gpdla_results_multi *results);

/* Per-quasar summary row of a multi-DLA batch -- every saved variable of multi :498-510 that is not
 * a per-sample array; the row a multi-GPU run all-gathers.  Layout, md =
 * max_dlas: min_z_dla, max_z_dla | log_prior_no_dla, log_prior_lls, log_prior_dla[md] |
 * log_likelihood_no_dla, log_likelihood_lls, log_likelihood_dla[md] | log_posterior_no_dla,
 * log_posterior_lls, log_posterior_dla[md] | model_posteriors[2+md] | p_no_dla, p_lls, p_dla |
 * MAP_z_dlas[md][md], MAP_log_nhis[md][md], MAP_inds[md][md] ([model][slot]) | all_exceptions
 * (1 or NaN, :139, :232).  78 columns for max_dlas = 4. */
#define GPDLA_SUMMARY_COLS_MULTI(md) (14 + 4 * (md) + 3 * (md) * (md))
int gpdla_batch_summary_multi_device_ptr(gpdla_batch *batch, double **table, int64_t *num_quasars,
                                         int32_t *num_cols);
/* Device pointers to the per-sample tables of a multi-DLA batch (valid after the first
 * gpdla_batch_process_multi): sample_log_likelihoods_dla [nq][max_dlas][S],
 * sample_log_likelihoods_lls [nq][S], base_sample_inds [nq][max_dlas-1][S].  Any may be NULL. */
int gpdla_batch_samples_multi_device_ptr(gpdla_batch *batch, double **sample_ll_dla,
                                         double **sample_ll_lls, uint32_t **base_sample_inds);

/* ---------------------------------------------------------------------------------------------
 * Training objective: objective.m:12-75 over spectrum_loss.m:14-76.
 * The training set stays resident in HBM; each call evaluates f(x) and g(x) = df/dx for
 * x = [vec M (G x k, column-major); log omega (G); log c0; log tau0; log beta] (objective.m:5),
 * including the Kim et al. priors the reference adds to the gradient (:59-71).
 * The three data matrices are [num_quasars x num_pixels] column-major as MATLAB holds them, NaN =
 * missing pixel (:42).  Returns GPDLA_ERR_NOT_POSITIVE_DEFINITE where chol would throw (:42).
 * ------------------------------------------------------------------------------------------- */
typedef struct gpdla_training gpdla_training;
int gpdla_training_create(int device_id, int64_t num_quasars, int64_t num_pixels,
                          const double *centered_rest_fluxes, const double *lya_1pzs,
                          const double *rest_noise_variances, gpdla_training **out);
int gpdla_training_objective(gpdla_training *t, const double *x, int k, double *f, double *g);
/* Switches the training set to the mean-flux model's objective, multi_dlas/objective_lyseries.m:12-78
 * over multi_dlas/spectrum_loss_lyseries.m:14-93 (what multi_dlas/learn_qso_model_meanflux.m:140-142
 * minimises): the optical depth of a pixel sums the first num_forest_lines Lyman lines, each counted
 * only where its redshift does not exceed the quasar's (zqso + 1 = the quasar's last lya_1pz,
 * objective_lyseries.m:46); everything else is objective.m.  all_transition_wavelengths (any unit,
 * decreasing) / all_oscillator_strengths: num_forest_lines entries each, or both NULL for the table
 * of set_parameters_multi.m:76-143 (include/gpdla_lyman_series.h).  num_forest_lines <= 1 switches
 * back to objective.m.  Takes effect from the next gpdla_training_objective call. */
int gpdla_training_set_lyseries(gpdla_training *t, int num_forest_lines, const double *all_transition_wavelengths,
                                const double *all_oscillator_strengths);
void gpdla_training_destroy(gpdla_training *t);

/* ---------------------------------------------------------------------------------------------
 * Learning the model from spectra: learn_qso_model.m:27-87 (single-DLA model) and
 * multi_dlas/learn_qso_model_meanflux.m:27-138 (mean-flux model) up to the PCA, on the GPU.  The
 * handle's three training matrices are made in HBM from the spectra, never on the host.
 * ------------------------------------------------------------------------------------------- */
/* The set_parameters.m / set_parameters_multi.m values the learning reads. */
typedef struct {
  double min_lambda, dlambda;       /* rest grid min_lambda + p dlambda, p < num_rest_pixels (:33-35) */
  int64_t num_rest_pixels;          /* G (1217 for the reference's grid) */
  double lya_wavelength;            /* set_parameters.m:5 */
  double max_noise_variance;        /* :37 (1; 9 for the mean-flux model) */
  double prev_tau_0, prev_beta;     /* learn_qso_model_meanflux.m:102-103 (0.0023, 3.65) */
  int32_t num_forest_lines;         /* <= 1: single-DLA model; 2..31: the mean-flux model over the
                                       built-in Lyman-series table (set_parameters_multi.m:75-144) */
} gpdla_learn_config;

/* A training set made from spectra (learn_qso_model.m:37-67, or learn_qso_model_meanflux.m:43-132 with
 * num_forest_lines > 1): each quasar interpolated onto the rest grid (NaN outside its range, NaN at
 * masked pixels), noisy pixels (rest noise variance > max_noise_variance) removed, and -- mean-flux
 * model -- flux and noise divided by the Lyman-series absorption exp(-tau) and exp(-tau)^2.  The
 * flux is NOT yet centred: gpdla_training_column_stats does that.  The prior pointers of `spectra` are
 * ignored.  gpdla_training_objective and gpdla_training_set_lyseries work on the result unchanged. */
int gpdla_training_create_from_spectra(int device_id, const gpdla_spectra *spectra, const gpdla_learn_config *config,
                                       gpdla_training **out);
/* Of a handle made by gpdla_training_create_from_spectra: mu = nanmean(rest_fluxes) (:70), the
 * centring of the resident flux in place (:71) and nanstd(centered_rest_fluxes) (:87, n - 1); count =
 * finite entries per pixel.  The first call centres; later calls return the same numbers.  Each
 * output [G] may be NULL. */
int gpdla_training_column_stats(gpdla_training *t, double *mu, double *std, int64_t *count);
/* The covariance pca(centered_rest_fluxes, 'rows', ...) decomposes: complete_rows = 0 for 'pairwise'
 * (learn_qso_model.m:75-78: cov_ab = Sum_q x_qa x_qb / (N_ab - 1) over the quasars finite in both
 * pixels), != 0 for 'complete' (learn_qso_model_meanflux.m:135-138: rows with any NaN dropped, the
 * rest centred by their own column mean, X'X / (n_c - 1)).  cov and count (N_ab; may be NULL) are
 * G x G, exactly symmetric; *rows_used (may be NULL): quasars with any finite pixel (pairwise) or the
 * complete rows.  Runs gpdla_training_column_stats first if it has not run. */
int gpdla_training_pca_covariance(gpdla_training *t, int complete_rows, double *cov, double *count,
                                  int64_t *rows_used);
/* The resident matrices, column-major [num_quasars x num_pixels] as MATLAB holds them (flux: centred
 * once column_stats has run).  Any pointer may be NULL. */
int gpdla_training_download(gpdla_training *t, double *flux, double *lya, double *noise);

/* ---------------------------------------------------------------------------------------------
 * Diagnostics.  The sweep kernel evaluates the Voigt function within 30 Doppler widths of a line
 * centre from per-line piecewise polynomials of Re w(x + i y_line) (what voigt.c:288 gets from
 * libcerf's voigt()).  This returns the HOST evaluation of the table of Lyman line `line`
 * (0 = Ly-alpha) at |x| < 32, and the line's damping parameter y = gamma/(sqrt2 sigma) in *y_out
 * (may be NULL).  Needs no GPU.
 * ------------------------------------------------------------------------------------------- */
int gpdla_debug_near_poly(int line, double x, double *value_out, double *y_out);

/* Test hook: runs only the preparation kernel of a batch (pixel selection, GP interpolation, noise
 * scaling; with multi != 0 the Lyman-series scaling and mean-flux suppression of
 * process_qsos_multiple_dlas_meanflux.m:245-293) and copies out, for quasar `quasar`, its rows on
 * the unmasked-range grid: rows_out[4 i + (0..3)] = (y, mu, omega2, nu) of pixel i (masked pixels:
 * 0, 0, 0, 1), for i < *num_rows_out <= capacity_rows.  Lets a test hold the GPU's mean-flux factor
 * to the numbers the reference's own QSOLoader.total_scale_factor produced (tests/golden/mean_flux.npz). */
int gpdla_debug_prepared_rows(gpdla_context *ctx, gpdla_batch *batch, int multi, int64_t quasar,
                              double *rows_out, int64_t capacity_rows, int64_t *num_rows_out);

/* The counter-based generator behind the multi-DLA resampling (Philox4x32-10 of Salmon et al.,
 * SC'11), evaluated on the HOST by the same function the kernel compiles: out = philox(ctr, key).
 * For known-answer tests against the Random123 vectors.  Needs no GPU. */
void gpdla_debug_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]);

/* Test hook for the boundary itself: throws, inside an entry point's body, std::bad_alloc (kind 1),
 * std::runtime_error (2) or a non-standard exception (3); kind 0 returns GPDLA_OK.  Every
 * int-returning entry point ends in the same handlers: the caller gets GPDLA_ERR_HOST and a message,
 * never a C++ exception (which would end MATLAB / Python).  Needs no GPU. */
int gpdla_debug_throw(int kind);

/* Test hook: what hipOccupancyMaxActiveBlocksPerMultiprocessor answers for a k <= 20 single-DLA sweep kernel
 * at its own launch shape (256 threads, 80 KiB of dynamic LDS).  kernel: 0 = k_sweep_slim<3>, 1 =
 * k_sweep_slim<0>, 2 = k_sweep_slim_boxed<3>, 3 = k_sweep_slim_boxed<0>.  The kernels are built for TWO blocks
 * per compute unit: the two waves of a SIMD belong to different blocks.  Needs a GPU. */
int gpdla_debug_slim_sweep_blocks_per_cu(int kernel, int *blocks_out);

/* ---------------------------------------------------------------------------------------------
 * CDDF statistics (CDDF_analysis/calc_cddf.py, class DLACatalogue).
 *
 * gpdla_stats_bin_posteriors: one pass over a block of selected spectra.  Row s of the sample
 * table starts at sample_log_likelihoods + s * row_stride (S values); p = exp(sll - shift[s]) *
 * p_dla[s] (shift = log_likelihoods_dla + log S, formed by the caller) and z = z_min[s] + (z_max[s]
 * - z_min[s]) * offset, each operation rounded on its own.  Each request bins z or log10 N_HI:
 *  - histogram = 0 (_split_distributions_single, :994-1034): samples with lnhi_lo < lnhi < lnhi_hi,
 *    z_lo < z < upper (upper = min(upper_z[s], z_hi) with lowzcut, else z_hi) and p >
 *    p_thresh_sample, in bin b when edges[b] < q < edges[b+1].  pois[s][b] sums those with p <
 *    p_switch; the others are kept as (bin, p) pairs in sample order, at most
 *    GPDLA_STATS_KEPT_CAPACITY per spectrum: kept_count[s] is the true number, and a spectrum above
 *    the capacity makes the call return GPDLA_ERR_UNSUPPORTED naming it (the outputs are written).
 *  - histogram != 0 (_get_z_nhi_hist, :1101-1125): the window without lowzcut and without a p cut,
 *    np.histogram's bins ([a, b), the last closed), mean[s][b] = sum w p and var[s][b] = sum w^2 (1 - p)
 *    p, w = 10^lnhi (moment != 0) or 1.  A NaN weight makes its bin and every later bin NaN, as
 *    np.histogram's cumulative sums do.
 * Every sum runs in sample order, compensated; outputs depend on their own row only.  Outputs are
 * [num_spectra][num_bins] and [num_spectra][GPDLA_STATS_KEPT_CAPACITY] (unused slots: bin -1, p 0);
 * pointers a request does not use may be NULL.  Edges must be finite and strictly increasing.
 *
 * gpdla_stats_poisson_binomial_cf: segment g holds p[offsets[g] .. offsets[g+1]) (N_g finite values
 * >= 0; a kept probability may exceed 1 by rounding, which is accepted); for n = 0 .. (N_g+1)/2 it writes logsum = sum_j log|1 + p_j (e^{-2 pi i n/(N_g+1)} - 1)| and
 * argsum = sum_j arg(...) (:1293-1295) at position n of the segment's block; the blocks follow one
 * another, (N_g+1)/2 + 1 values each.  The pdf is irfft(exp(logsum + i argsum), N_g + 1).
 * ------------------------------------------------------------------------------------------- */
#define GPDLA_STATS_MAX_BINS 64
#define GPDLA_STATS_MAX_REQUESTS 4
#define GPDLA_STATS_KEPT_CAPACITY 8
typedef struct {
  int32_t quantity;       /* 0: z, 1: log10 N_HI */
  int32_t num_bins;       /* 1 .. GPDLA_STATS_MAX_BINS */
  const double *edges;    /* [num_bins + 1] */
  double z_lo, z_hi, lnhi_lo, lnhi_hi;
  int32_t histogram, moment, lowzcut;
  double p_thresh_sample, p_switch;
} gpdla_bin_request;
typedef struct {
  double *pois, *mean, *var;   /* [num_spectra][num_bins] */
  int32_t *kept_count;         /* [num_spectra] */
  int32_t *kept_bin;           /* [num_spectra][GPDLA_STATS_KEPT_CAPACITY] */
  double *kept_p;
} gpdla_bin_output;
int gpdla_stats_bin_posteriors(int64_t num_spectra, int64_t num_samples, const double *sample_log_likelihoods,
                               int64_t row_stride, const double *shift, const double *p_dla, const double *z_min,
                               const double *z_max, const double *upper_z, const double *offset_samples,
                               const double *log_nhi_samples, int num_requests, const gpdla_bin_request *requests,
                               gpdla_bin_output *outputs, int device_id);
int gpdla_stats_poisson_binomial_cf(int64_t num_segments, const int64_t *offsets, const double *p, double *logsum,
                                    double *argsum, int device_id);

/* gpdla_stats_bin_posteriors for the rows of a refine pass.  Additive: GPDLA_ABI_VERSION is
 * unchanged.  Row s holds lambda_j, j < S' (sample_log_posteriors_refined, at sample_log_posteriors + s *
 * row_stride); boxes[s] = (z_lo, z_hi, n_lo, n_hi) is the row's box of the last level; u, v are the shared
 * unit points, each inside [0, 1).  Per row, each operation rounded on its own:
 *   shift[s] = m + log(Sum_j exp(lambda_j - m)), m = the maximum of the row, NaN entries skipped by both; a
 *              row without a finite entry, or with +inf, has shift NaN.  The sum is compensated and runs in an
 *              order fixed by S' alone.
 *   p_j = exp(lambda_j - shift[s]) * p_dla[s],  z_j = z_lo + (z_hi - z_lo) u_j,  lnhi_j = n_lo + (n_hi - n_lo)
 *   v_j,  w_j = exp10(lnhi_j) (the N' the boxed sweep itself used, where gpdla_stats_bin_posteriors takes the
 *   host's pow).
 * The requests, every comparison, the kept-pair rule and its capacity, the NaN poisoning of histogram bins
 * and the output layouts are gpdla_stats_bin_posteriors'.  A NaN shift makes every p of the row NaN, and the
 * row is treated as that entry treats NaN p.  A zero-width box is legal.  No atomics: a row's outputs depend
 * on that row only and are bit-identical from run to run and for any blocking of the rows.  The argument
 * checks (null pointers, row_stride < S', edges, the number of requests, u or v outside [0, 1)) run before
 * the device is touched and need no GPU. */
int gpdla_stats_bin_posteriors_boxed(int64_t num_rows, int64_t num_points, const double *sample_log_posteriors,
                                     int64_t row_stride, const double *p_dla, const double *boxes, const double *upper_z,
                                     const double *u, const double *v, int num_requests,
                                     const gpdla_bin_request *requests, gpdla_bin_output *outputs, double *shift,
                                     int device_id);
/* Measuring aids for tools/bench_refined_stats.py.  gpdla_debug_time_bin_kernels(1) makes the calling thread's
 * later calls of the two entries above bracket their kernel launch with device events (0: off, the default --
 * a call then launches as it always did); gpdla_debug_last_bin_ms returns the duration of the k_bin_posteriors
 * or k_bin_posteriors_boxed launch of that thread's most recent timed call (-1 before the first). */
void gpdla_debug_time_bin_kernels(int on);
double gpdla_debug_last_bin_ms(void);

/* ---------------------------------------------------------------------------------------------
 * Sightline S/N, path length per sightline and bin, stratified bootstrap.  Additive:
 * GPDLA_ABI_VERSION is unchanged.
 *
 * gpdla_stats_sightline_snrs: find_snr of calc_cddf.py:1167-1185 as it executes, on ragged CSR
 * spectra (sightline i holds pixels offsets[i] .. offsets[i+1]).  The pixels with wavelength >
 * 1215.67 * (1 + max_z_dlas[i]) are taken, masked or not; flux with flux / normalizers[i] < 0.1
 * becomes normalizers[i] * 0.1 (normalizers == NULL: flux < 0.1 becomes 0.1); snrs[i] = 1 /
 * median(sqrt(noise_variance) / |flux|), the median as NumPy takes it: NaN if any selected value is
 * NaN or none is selected (a NaN max_z_dla selects none), the mean of the middle two for an even
 * count.  Any number of selected pixels is handled.
 *
 * gpdla_stats_path_lengths: dX[i][b] = integral of (1+z)^2 / sqrt(omega_m (1+z)^3 + 1 - omega_m) over
 * the overlap of [min_z_dlas[i], hi_i] with [edges[b], edges[b+1]]; hi_i = max_z_dlas[i], or with
 * lowzcut max(min(hi, hi - proximity_zone), min_z_dlas[i]).  A sightline with min >= edges[b+1] or
 * hi <= edges[b] (or a NaN end) gets exactly 0.  8-node Gauss-Legendre on panels no wider than 0.25.
 * A search range that ends below its start is GPDLA_ERR_INVALID_ARGUMENT.  1 .. GPDLA_STATS_MAX_BINS bins.
 *
 * gpdla_stats_bootstrap_sums: V is [num_rows][num_columns] (1 .. GPDLA_BOOTSTRAP_MAX_COLUMNS columns),
 * its rows sorted by stratum[] (non-decreasing labels >= 0).  For replicate r = first_replicate ..
 * first_replicate + num_replicates - 1, position j (0 .. num_rows - 1, in a stratum that starts at
 * row f and holds m rows) draws row f + ((uint64) w * m >> 32), w the first word of Philox4x32-10 at
 * counter (lo32(j), hi32(j), r, 2) under key (lo32(seed), hi32(seed)); sums[r - first_replicate][c]
 * is the compensated sum of V[row][c] over the positions in a fixed order.  A replicate's sums do
 * not depend on first_replicate / num_replicates of the call that computed it.
 * ------------------------------------------------------------------------------------------- */
#define GPDLA_BOOTSTRAP_MAX_COLUMNS 256
int gpdla_stats_sightline_snrs(int64_t num_sightlines, const int64_t *offsets, const double *wavelengths,
                               const double *flux, const double *noise_variance, const double *max_z_dlas,
                               const double *normalizers, double *snrs, int device_id);
int gpdla_stats_path_lengths(int64_t num_sightlines, const double *min_z_dlas, const double *max_z_dlas,
                             int num_bins, const double *edges, int lowzcut, double proximity_zone, double omega_m,
                             double *dX, int device_id);
int gpdla_stats_bootstrap_sums(int64_t num_rows, int num_columns, const double *V, const int32_t *stratum,
                               uint64_t seed, int64_t first_replicate, int64_t num_replicates, double *sums,
                               int device_id);

/* ---------------------------------------------------------------------------------------------
 * Model spectra: what the fitted model looks like on a spectrum -- the numbers
 * behind the reference's QSOLoader.plot_this_mu (CDDF_analysis/qso_loader.py:1654-1774) and the
 * per-pixel quantities a processed sample table stands for.
 *
 * Per-pixel outputs live on a quasar's UNMASKED-RANGE GRID: every stored pixel whose rest wavelength
 * lies in [min_lambda, max_lambda] (process_qsos.m:104-108), masked or not, in stored order -- n_u
 * pixels, the grid the Voigt stage of the sweeps runs on (padded by 3 pixels a side at
 * pixel_spacing, :168-176).  Output arrays are CSR-style: offsets[num_selected + 1] (written by the
 * call) and one value per grid pixel of each selected quasar, in selection order.
 *
 *  map_absorption   Prod_j of the instrument-broadened Voigt profiles of the quasar's listed absorbers
 *                   (z_j, N_j) with the context's num_lines: the `absorption` vector of
 *                   process_qsos.m:187-190 before the mask drop, multiplied over absorbers (multi
 *                   :342-351).  Ones for an empty list; NaN for a quasar without a kept pixel (it has
 *                   no padded grid).
 *  mean_absorption, var_absorption
 *                   posterior-weighted mean and variance, over all S samples, of the broadened profile
 *                   of sample i: z_i = min_z_dla + (max_z_dla - min_z_dla) offset_i, N_i = nhi_samples[i]
 *                   (sub_dla: lls_nhi_samples[i]), weights w_i = exp(l_i - max l) / Sum from a row l of
 *                   sample log-likelihoods; a NaN l_i weighs 0, an all-NaN row gives NaN.  The row is
 *                   the batch's resident table after gpdla_batch_process / gpdla_batch_process_multi
 *                   (multi-DLA batch: model DLA(1), or the sub-DLA table with sub_dla), or row s of
 *                   the caller's host table sample_log_likelihoods[num_selected][S] -- a processed file
 *                   needs no second sweep.  Models with two or more absorbers:
 *                   gpdla_batch_model_spectra_multi.
 *  continuum, model_flux
 *                   with a = map_absorption (ones for an empty list) and the prepared rows y, mu, M,
 *                   omega2, nu of the kept pixels (meanflux != 0: with the Lyman-series suppression of
 *                   multi :245-293): d = a^2 omega2 + nu, r = y - a mu, B = I + M' diag(a^2/d) M,
 *                   c = B^-1 M' (a r / d); continuum = mu + M c at ALL n_u pixels (a masked pixel takes
 *                   the same interpolated mu and M), model_flux = a continuum.  This is the posterior
 *                   mean of the LOW-RANK part of the GP; the pixel-diagonal omega term predicts nothing
 *                   at a pixel that was not measured and is left out.  B not positive definite: NaN
 *                   rows and status 4 for that quasar, the call still returns GPDLA_OK.
 *
 * Sums run in a fixed order without atomics: outputs are bit-identical from run to run, for any
 * selection order and any batching, and for the resident and the host form of the same table.
 * The call returns when the outputs are in the caller's arrays.
 *
 * THE REFINED SOURCE (GPDLA_SPECTRA_WEIGHTS_REFINED; additive, GPDLA_ABI_VERSION unchanged).  After
 * gpdla_batch_refine with L levels on the context's S' refine points (u_j, v_j), a quasar q of refine status 0 has its
 * last box (z_lo, z_hi, n_lo, n_hi) = boxes[q][L-1] and the resident table lambda_j =
 * sample_log_posteriors_refined[q][j].  Its refined sample j is z'_j = z_lo + (z_hi - z_lo) u_j, N'_j =
 * exp10(n_lo + (n_hi - n_lo) v_j), in the arithmetic of the boxed sweep that produced l'_j.  With the refined source,
 * mean_absorption and var_absorption are their definitions above with (S, offset_i, N_i, l, min_z_dla, max_z_dla) replaced
 * by (S', u, N', lambda, z_lo, z_hi): the weights are exp(lambda_j - max) / Sum, a NaN weighs 0, an entry the separation
 * mask set to -inf weighs 0.  Posterior mass outside the last box is ignored -- the convention of the refined parameter
 * summaries.  The refined table is the DLA table: sub_dla != 0 is refused with it.  The call returns
 * GPDLA_ERR_INVALID_ARGUMENT when the batch has not been refined or the context's refine points changed since.  A selected
 * quasar whose refine status is not 0 (outside the refine's selection, or unusable) gets NaN rows and the status bit
 * GPDLA_SPECTRA_NOT_REFINED.  The promise of fixed-order sums holds as above.
 * ------------------------------------------------------------------------------------------- */
#define GPDLA_SPECTRA_MAX_ABSORBERS 8
#define GPDLA_SPECTRA_MAP 1        /* products bit: map_absorption */
#define GPDLA_SPECTRA_MOMENTS 2    /* mean_absorption and var_absorption */
#define GPDLA_SPECTRA_CONTINUUM 4  /* continuum and model_flux */
#define GPDLA_SPECTRA_WEIGHTS_NONE 0
#define GPDLA_SPECTRA_WEIGHTS_RESIDENT 1
#define GPDLA_SPECTRA_WEIGHTS_HOST 2
#define GPDLA_SPECTRA_WEIGHTS_REFINED 3  /* the resident refined table of gpdla_batch_refine (the DLA table only) */
#define GPDLA_SPECTRA_NOT_REFINED 16     /* status bit: refined source, the quasar has no refined table (NaN rows) */
typedef struct {
  int64_t num_selected;
  const int64_t *selection;          /* [num_selected] quasars of the batch; NULL = 0 .. num_selected-1 */
  const int64_t *absorber_offsets;   /* [num_selected + 1] into absorber_z / absorber_nhi; NULL = no absorbers */
  const double *absorber_z;
  const double *absorber_nhi;        /* column densities (not their logarithms) */
  int32_t weights_source;            /* GPDLA_SPECTRA_WEIGHTS_* */
  const double *sample_log_likelihoods; /* [num_selected][S], GPDLA_SPECTRA_WEIGHTS_HOST */
  int32_t sub_dla;                   /* != 0: lls_nhi_samples (and the resident sub-DLA table) */
  int32_t meanflux;                  /* != 0: prepared rows of the mean-flux model (multi :245-293) */
  int32_t products;                  /* GPDLA_SPECTRA_MAP | _MOMENTS | _CONTINUUM */
  int64_t capacity;                  /* entries of each per-pixel output array */
} gpdla_model_spectra_request;
typedef struct {
  int64_t *offsets;                  /* [num_selected + 1]; required */
  double *map_absorption, *mean_absorption, *var_absorption, *continuum, *model_flux; /* any may be NULL */
  int32_t *status;                   /* [num_selected] or NULL: the quasar's sweep status (0, 1, 3), or 4 = B not
                                        positive definite (continuum) */
} gpdla_model_spectra;

/* The checks gpdla_batch_model_spectra makes before its first device call, for a batch of num_quasars
 * quasars and S = num_samples: more than GPDLA_SPECTRA_MAX_ABSORBERS absorbers for a quasar or
 * decreasing absorber_offsets, a selection index outside the batch, moments without a weights source
 * (or a host source without a table), sub_dla without lls_nhi_samples, no product or an unknown one.
 * Returns GPDLA_OK or GPDLA_ERR_INVALID_ARGUMENT.  Needs no GPU. */
int gpdla_model_spectra_validate(const gpdla_model_spectra_request *request, int64_t num_quasars,
                                 int64_t num_samples, int has_lls_nhi_samples);
/* n_u of every quasar of the batch (runs the preparation kernel; synchronises): the sizes a caller
 * allocates the outputs of gpdla_batch_model_spectra from. */
int gpdla_batch_unmasked_counts(gpdla_context *ctx, gpdla_batch *batch, int64_t *n_u);
int gpdla_batch_model_spectra(gpdla_context *ctx, gpdla_batch *batch, const gpdla_model_spectra_request *request,
                              gpdla_model_spectra *out);

/* With gpdla_context_set_timing enabled, gpdla_context_last_sweep_ms reports the k_spectra_moments +
 * k_spectra_combine launches of the most recent gpdla_batch_model_spectra call that computed moments.
 *
 * Measuring aid for tools/bench_model_spectra.py: runs the preparation kernel and then k_profiles ALONE
 * over every quasar of a multi-DLA batch (the Voigt stage of the multi-DLA driver: the same line sums,
 * 2 S n values stored instead of reduced) and returns the k_profiles launches' duration from device
 * events.  The batch's results are untouched; the context's profile table is overwritten. */
int gpdla_debug_profiles_ms(gpdla_context *ctx, gpdla_batch *batch, double *ms_out);

/* The reference's `this_mu` (qso_loader.py:1685-1711) as data, on the model's rest grid: for item i,
 * out[i][g] = mu[g] x (suppressed != 0: QSOLoader.total_scale_factor(prev_tau_0, prev_beta, z_qsos[i],
 * rest_wavelengths, num_forest_lines)[g], :1777-1822) x Prod_j Voigt_absorption(rest_wavelengths (1 +
 * z_qsos[i]), absorber_nhi[j], absorber_z[j], num_voigt_lines)[g] -- RAW profiles, no instrument
 * broadening -- over the item's absorbers j in absorber_offsets[i] .. absorber_offsets[i+1] (at most
 * GPDLA_SPECTRA_MAX_ABSORBERS; absorber_offsets NULL = none).  Only num_rest_pixels, rest_wavelengths
 * and mu of `model` are read.  Line counts in [1, 31].  Invalid arguments are refused before any device
 * call. */
int gpdla_model_mean(const gpdla_model *model, int64_t num_items, const double *z_qsos,
                     const int64_t *absorber_offsets, const double *absorber_z, const double *absorber_nhi,
                     int num_voigt_lines, int num_forest_lines, int suppressed, double prev_tau_0,
                     double prev_beta, double *out, int device_id);

/* ---------------------------------------------------------------------------------------------
 * Model spectra of a multi-DLA run: the per-pixel absorption averaged over the samples of
 * every model and over the models.  Additive: GPDLA_ABI_VERSION is unchanged.  Everything lives on the
 * quasar's unmasked-range grid of gpdla_batch_model_spectra, in the same CSR layout; the padded
 * wavelengths, z_i = min_z_dla + (max_z_dla - min_z_dla) offset_i, nhi_samples, the context's num_lines and
 * the seven taps are those of mean_absorption there.
 *
 * Per entry s of the selection (quasar q), model n = 1 .. max_dlas, sample i = 0 .. S-1:
 *  slots    s_1(i) = i;  s_j(i) = base_sample_inds[q][j-2][i] - 1 for j = 2 .. n  (1-based uint32,
 *           [nq][max_dlas-1][S]: the rule of gpdla_stats_parameter_summaries)
 *  profile  A_{n,i}(p) = Prod_{j=1..n} c_{s_j(i)}(p), c_s the instrument-BROADENED profile of sample s
 *           (multi :342-351: a product of convolved profiles, not the convolution of a product),
 *           multiplied in slot order
 *  weights  w_i = exp(l_i - max l) / Sum from row sample_log_likelihoods_dla[q][n-1][.]: a NaN l_i weighs
 *           0; a sample one of whose slots j >= 2 has base index 0 ("never drawn") is read as a NaN l_i
 *           whatever its log-likelihood says; a row with nothing above -inf, or with a +inf entry, is
 *           FLAGGED: NaN rows for that model, bit (n-1) of model_flags[s]
 *  moments  mean_n(p) = Sum_i w_i A_{n,i}(p), var_n(p) = Sum_i w_i (A_{n,i}(p) - mean_n(p))^2, accumulated
 *           as mb = Sum w b and m2 = Sum w b^2 of the absorbed fraction b = 1 - A: mean = 1 - mb, var =
 *           max(m2 - mb^2, 0).  Model DLA(1) is mean_absorption / var_absorption of
 *           gpdla_batch_model_spectra for the same row, bit for bit; the sub-DLA model is its sub_dla form
 *           (lls_nhi_samples, the sub-DLA table; flagged: GPDLA_SPECTRA_MULTI_FLAG_LLS of model_flags[s])
 *  average  with model weights P = (P_null, P_lls, P_1 .. P_md) (row s of model_weights, or the batch's
 *           resident model_posteriors of quasar q):
 *             Eb(p) = P_lls mb_lls(p) + Sum_n P_n mb_n(p),  Eb2(p) = P_lls m2_lls(p) + Sum_n P_n m2_n(p)
 *           added in the order sub-DLA, DLA(1), .., DLA(md) (the null model absorbs nothing):
 *             expected_absorption = 1 - Eb,  expected_var_absorption = max(Eb2 - Eb^2, 0)
 *           A model with P_m == 0 is skipped even if it is flagged.  A NaN entry of P, or P_m != 0 on a
 *           flagged model, makes the entry's two rows NaN and sets GPDLA_SPECTRA_AVERAGE_UNDEFINED in
 *           status[s] -- the early exit of the reference leaves a whole model_posteriors row NaN, and
 *           nothing here papers over it.
 * A quasar without a usable sweep (status 1 or 3) has NaN rows everywhere.
 *
 * Sums run in a fixed order without atomics: outputs are bit-identical from run to run, for any
 * selection order and grouping, and for the resident and the host form of the same tables.
 * ------------------------------------------------------------------------------------------- */
#define GPDLA_SPECTRA_MULTI_MODELS 1   /* products bit: the per-model rows and the sub-DLA rows */
#define GPDLA_SPECTRA_MULTI_AVERAGE 2  /* expected_absorption and expected_var_absorption */
#define GPDLA_SPECTRA_AVERAGE_UNDEFINED 8        /* status bit */
#define GPDLA_SPECTRA_MULTI_FLAG_LLS 0x40000000u /* model_flags bit of the sub-DLA model */
typedef struct {
  int64_t num_selected;
  const int64_t *selection;          /* [num_selected] quasars of the batch; NULL = 0 .. num_selected-1 */
  int32_t max_dlas;                  /* models of the tables: 1 .. GPDLA_POSTERIOR_MAX_MODELS */
  int32_t first_model, last_model;   /* the models whose rows are returned, 1 <= first <= last <= max_dlas */
  int32_t tables_source;             /* GPDLA_SPECTRA_WEIGHTS_RESIDENT (after gpdla_batch_process_multi) or _HOST */
  const double *sample_log_likelihoods_dla;  /* host: [num_selected][max_dlas][S] */
  const uint32_t *base_sample_inds;          /* host: [num_selected][max_dlas-1][S], 1-based, 0 = never drawn;
                                                may be NULL when max_dlas == 1 */
  const double *sample_log_likelihoods_lls;  /* host: [num_selected][S] */
  const double *model_weights;       /* host [num_selected][2 + max_dlas], or NULL: the resident model_posteriors */
  int32_t meanflux;                  /* != 0: prepared rows of the mean-flux model */
  int32_t products;                  /* GPDLA_SPECTRA_MULTI_MODELS | _AVERAGE */
  int64_t capacity;                  /* entries of each per-pixel output plane */
} gpdla_model_spectra_multi_request;
typedef struct {
  int64_t *offsets;                  /* [num_selected + 1]; required */
  double *mean_absorption_models, *var_absorption_models; /* [max_dlas][capacity]: plane n-1 is model DLA(n); NaN
                                                             outside first_model .. last_model; either may be NULL */
  double *mean_absorption_lls, *var_absorption_lls;       /* [capacity] or NULL */
  double *expected_absorption, *expected_var_absorption;  /* [capacity] or NULL */
  int32_t *status;                   /* [num_selected] or NULL: the quasar's sweep status (0, 1, 3), with
                                        GPDLA_SPECTRA_AVERAGE_UNDEFINED where the average is */
  uint32_t *model_flags;             /* [num_selected] or NULL: bit n-1 = model DLA(n) has no weight */
} gpdla_model_spectra_multi;

/* The checks gpdla_batch_model_spectra_multi makes before its first device call, for a batch of num_quasars
 * quasars uploaded for batch_max_dlas models (0: a single-DLA batch) that has (batch_processed != 0) or has
 * not run gpdla_batch_process_multi: models outside 1 .. max_dlas, a resident source on a single-DLA batch,
 * on a batch of another max_dlas or on one that has not been processed, host tables with a missing pointer,
 * a host base index above num_samples, the average of host tables without model_weights, no product or an
 * unknown one, a selection index outside the batch, no lls_nhi_samples.  Returns GPDLA_OK or
 * GPDLA_ERR_INVALID_ARGUMENT.  Needs no GPU. */
int gpdla_model_spectra_multi_validate(const gpdla_model_spectra_multi_request *request, int64_t num_quasars,
                                       int64_t num_samples, int has_lls_nhi_samples, int batch_max_dlas,
                                       int batch_processed);
/* The selected quasars are taken in groups whose partial sums (every model's) fit 256 MiB; results do not
 * depend on the grouping.  With gpdla_context_set_timing enabled, gpdla_context_last_sweep_ms reports the
 * weights, moments, combine and average launches of the most recent call.  A batch conditioned on fixed
 * absorbers is refused with GPDLA_ERR_UNSUPPORTED. */
int gpdla_batch_model_spectra_multi(gpdla_context *ctx, gpdla_batch *batch,
                                    const gpdla_model_spectra_multi_request *request, gpdla_model_spectra_multi *out);

/* ---------------------------------------------------------------------------------------------
 * Mock spectra: one draw per quasar of a resident batch from the distribution
 * whose likelihood the sweeps evaluate (process_qsos.m:190-198),
 *     flux ~ N(a mu, A (M M' + diag omega2) A + diag nu),   A = diag a,
 * on the KEPT pixels of the quasar's unmasked-range grid: a = the instrument-broadened product of the
 * listed absorbers (what gpdla_batch_model_spectra returns as map_absorption; ones for an empty
 * list), mu, M, omega2 = the rows the preparation kernel hands the sweep (meanflux != 0: the
 * Lyman-series rows of multi :245-293), nu = the stored noise variance.
 *     z     in R^k  standard normal, one vector per quasar            (stream 0, index i = 0 .. k-1)
 *     eps_j         standard normal per STORED pixel position j       (stream 1, index j)
 *     continuum_p = mu_p + M_p. z;  sigma_p = sqrt(a_p^2 omega2_p + nu_p);  flux_p = a_p continuum_p + sigma_p eps_p
 * Normals: Philox4x32-10, counter (lo32(index), hi32(index), stream, 1) -- the multi-DLA resampling
 * uses counter word 3 = 0, so the streams are disjoint under one seed -- and key
 * (seed ^ qid, (seed >> 32) ^ (qid >> 32) ^ 0x5851F42D), qid = first_quasar_index + q.  From the four
 * output words m1 = (out0 >> 5) 2^26 + (out1 >> 6), m2 likewise from out2, out3; u1 = (m1 + 1) 2^-53,
 * u2 = m2 2^-53, n = sqrt(-2 ln u1) cos(2 pi u2): one normal per call, |n| <= 8.58.  eps is indexed by
 * the stored position, so a quasar's draw depends neither on its mask nor on the batching.
 * Pixels that are not drawn: a stored pixel outside [min_lambda, max_lambda] keeps the uploaded flux
 * (masked or not: the model says nothing there); a masked pixel inside gets NaN (flux, continuum,
 * sigma); a quasar of status != 0 keeps its flux, reports its status, and has NaN continuum, sigma
 * and latents.  A kept pixel the sweep sees as a neutral row (noise variance above 1e100) is drawn as
 * pure noise of its stored variance.  Nothing is accumulated with atomics and every sum runs in a
 * fixed order: outputs are bit-identical from run to run.
 * With write_resident != 0 the batch's resident flux becomes the draw: a following
 * gpdla_batch_process / gpdla_batch_process_multi sweeps it without the flux visiting the host.
 * The call returns when the outputs are in the caller's arrays.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  uint64_t seed;
  const int64_t *absorber_offsets;   /* [num_quasars + 1] or NULL: no absorbers */
  const double *absorber_z, *absorber_nhi;   /* <= GPDLA_SPECTRA_MAX_ABSORBERS per quasar; N, not log N */
  int32_t meanflux;                  /* rows of the mean-flux model */
  int32_t write_resident;            /* != 0: the batch's resident flux is replaced by the draw */
  int64_t capacity_stored, capacity_grid;   /* entries of flux; of each per-grid-pixel array */
} gpdla_mock_request;
typedef struct {
  double *flux;                      /* [stored pixels of the batch], upload layout; may be NULL */
  int64_t *grid_offsets;             /* [num_quasars + 1]; required */
  double *absorption, *continuum, *sigma;   /* per grid pixel; any may be NULL */
  double *latents;                   /* [num_quasars][k] or NULL */
  int32_t *status;                   /* [num_quasars] or NULL: the quasar's sweep status (0, 1, 3) */
} gpdla_mock_spectra;
/* The checks gpdla_batch_draw_mocks makes before its first device call: more than
 * GPDLA_SPECTRA_MAX_ABSORBERS absorbers for a quasar, decreasing absorber_offsets, a NaN redshift, a
 * column density that is NaN or not positive, a negative capacity.  Needs no GPU. */
int gpdla_mock_validate(const gpdla_mock_request *request, int64_t num_quasars);
int gpdla_batch_draw_mocks(gpdla_context *ctx, gpdla_batch *batch, const gpdla_mock_request *request,
                           gpdla_mock_spectra *out);

/* ---------------------------------------------------------------------------------------------
 * DLA parameter samples and LLS normalisers: what generate_dla_samples.m,
 * multi_dlas/generate_dla_samples_multi.m and multi_dlas/set_lls_parameters.m compute from the
 * catalogue's log10 N_HI values.  Additive: GPDLA_ABI_VERSION is unchanged.  Every pointer is the
 * caller's, in host memory; arguments are checked before the GPU is touched.
 *
 * gpdla_samples_kde: density[g] = 1 / (N h) Sum_j phi((points[g] - values[j]) / h), phi the standard
 * normal density, no boundary correction (ksdensity's defaults).  bandwidth > 0 is used as given;
 * bandwidth == 0 takes h = sig (4 / (3 N))^(1/5), sig = median(|v - median(v)|) / 0.6745, and
 * sig == 0 is GPDLA_ERR_INVALID_ARGUMENT.  *bandwidth_used (optional) receives h.  N >= 2, any
 * num_points >= 0.  The sums run in a fixed order: the result depends on the inputs only.
 *
 * gpdla_nhi_prior: p(t) = alpha g(t) / Z + (1 - alpha) U[uniform_min, uniform_max](t) on
 * [lower, GPDLA_SAMPLES_UPPER], log g(t) = coeff[0] + coeff[1] s + coeff[2] s^2 with s = t - centre;
 * with a finite flat_below, g(t) = g(flat_below) for t < flat_below (NaN: no such break);
 * Z = integral of g over [lower, GPDLA_SAMPLES_UPPER]; F(x) = integral of p over [lower, x].
 *
 * gpdla_samples_fit_prior: the KDE of `values` on GPDLA_SAMPLES_FIT_POINTS equally spaced points of
 * [fit_min, fit_max] (bandwidth as above), the least-squares quadratic through its logarithm (about
 * centre = (fit_min + fit_max) / 2, by orthogonal polynomials), and Z.  The other fields of *prior are
 * copied from the arguments.  A KDE that underflows to 0 on the grid is GPDLA_ERR_INVALID_ARGUMENT.
 *
 * gpdla_samples_prior_eval: pdf[i] = p(x[i]) and cdf[i] = F(x[i]) (either may be NULL); F is 0 at and
 * below lower and F(GPDLA_SAMPLES_UPPER) at and above the upper limit.
 *
 * gpdla_samples_halton: out[i][d] = Sum_j pi_b(d_j) b^-(j+1) for b = bases[d] (2 .. GPDLA_HALTON_MAX_BASE,
 * at most GPDLA_HALTON_MAX_DIMS of them), d_j the base-b digits of index first_index + i, pi_b the
 * reverse-radix ("RR2") permutation: the ceil(log2 b)-bit bit reversals of 0, 1, 2, ... in order,
 * those >= b dropped.  Each value is the correctly rounded quotient of two exact integers.  Index 0
 * is the origin.  first_index >= 0 and first_index + num <= 2^32.
 *
 * gpdla_samples_draw: sample i (index first_index + i) takes the points of bases 2, 3, 5 -- or row i
 * of `sequence` ([num][sequence_dims], sequence_dims 2 or 3, values in [0, 1]) -- as (u1, u2, u3):
 * offset = u1, log_nhi = F^-1(u2) (u2 == 0: lower exactly; u2 >= F(upper): the upper limit; else
 * |F(x) - u2| <= 1e-13 or x bracketed to one ulp), nhi = 10^log_nhi, and when out->lls_nhi is given
 * lls_offset = u3, lls_log_nhi = lls_lower + (lls_upper - lls_lower) u3, lls_nhi = 10^lls_log_nhi.
 * ------------------------------------------------------------------------------------------- */
#define GPDLA_SAMPLES_UPPER 25.0
#define GPDLA_SAMPLES_FIT_POINTS 1000
#define GPDLA_HALTON_MAX_DIMS 8
#define GPDLA_HALTON_MAX_BASE 64
typedef struct {
  double coeff[3];                   /* log g about `centre`: constant, linear, quadratic */
  double centre;
  double alpha;                      /* in [0, 1] */
  double uniform_min, uniform_max;
  double lower;                      /* F(lower) = 0 */
  double flat_below;                 /* NaN: none */
  double Z;
} gpdla_nhi_prior;
typedef struct {
  double *offset, *log_nhi, *nhi;               /* [num]; required */
  double *lls_offset, *lls_log_nhi, *lls_nhi;   /* [num]; all three or none */
} gpdla_sample_draw;
int gpdla_samples_kde(int64_t num_values, const double *values, int64_t num_points, const double *points,
                      double bandwidth, double *density, double *bandwidth_used, int device_id);
int gpdla_samples_fit_prior(int64_t num_values, const double *values, double fit_min, double fit_max, double alpha,
                            double uniform_min, double uniform_max, double lower, double flat_below,
                            double bandwidth, gpdla_nhi_prior *prior, int device_id);
int gpdla_samples_prior_eval(const gpdla_nhi_prior *prior, int64_t num_points, const double *x, double *pdf,
                             double *cdf, int device_id);
int gpdla_samples_halton(int64_t first_index, int64_t num, int num_bases, const int32_t *bases, double *out,
                         int device_id);
int gpdla_samples_draw(const gpdla_nhi_prior *prior, int64_t first_index, int64_t num, const double *sequence,
                       int sequence_dims, double lls_lower, double lls_upper, gpdla_sample_draw *out,
                       int device_id);

/* ---------------------------------------------------------------------------------------------
 * Preloading spectra: the columns of SDSS spec files -> the normalised, truncated
 * spectra of preloaded_qsos.mat, as read_spec.m:27-38 and preload_qsos.m:26-67 compute them.
 * Additive: GPDLA_ABI_VERSION is unchanged.
 *
 * Input: a raw CSR set (quasar i holds pixels offsets[i] .. offsets[i+1]) of the float32 columns
 * flux, loglam, ivar and the int32 column and_mask, one redshift per quasar, and filter_flags[]
 * (in/out).  A quasar whose flag is not 0 on entry is not looked at.  For the others, per pixel in
 * fp64: wavelength = 10^loglam, noise_variance = 1 / ivar, pixel_mask = (ivar == 0) | bit 23 of
 * and_mask (0-based; MATLAB's bitget(and_mask, 24)), rest = wavelength / (1 + z).  normalizers[i] =
 * the median of the non-NaN flux of the unmasked pixels with rest in [normalization_min_lambda,
 * normalization_max_lambda] (mean of the middle two for an even count); none: filter_flags[i] |= 4.
 * Fewer than min_num_pixels unmasked pixels with rest in [min_lambda, max_lambda]: filter_flags[i]
 * |= 8.  A quasar flagged on entry or here keeps no pixel and normaliser 0.  Otherwise the pixels
 * with rest in [loading_min_lambda, loading_max_lambda], masked or not, plus the nearest unmasked
 * pixel below the first and above the last of them (where one exists) are kept in pixel order, with
 * flux / normaliser and noise_variance / normaliser^2.
 *
 * Output: CSR (out_offsets[num_quasars + 1]) wavelengths, flux, noise_variance, pixel_mask; the
 * caller sizes these four by the INPUT pixel count offsets[num_quasars].  Bit-identical run to run
 * and independent of how a set is split into calls.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  double loading_min_lambda, loading_max_lambda;             /* set_parameters.m:21-22 */
  double normalization_min_lambda, normalization_max_lambda; /* :29-30 */
  double min_lambda, max_lambda;                             /* :33-34 */
  int64_t min_num_pixels;                                    /* :26 */
} gpdla_preload_config;
int gpdla_preload_spectra(int64_t num_quasars, const int64_t *offsets, const float *flux, const float *loglam,
                          const float *ivar, const int32_t *and_mask, const double *z_qsos, uint8_t *filter_flags,
                          const gpdla_preload_config *config, int64_t *out_offsets, double *wavelengths,
                          double *out_flux, double *noise_variance, uint8_t *pixel_mask, double *normalizers,
                          int device_id);

/* ---------------------------------------------------------------------------------------------
 * Credible intervals and moments of the absorber parameters.  Additive:
 * GPDLA_ABI_VERSION is unchanged.
 *
 * A row of S sample log-likelihoods l_i of model m (m absorbers, m = 1 .. num_models) is a weighted
 * sample of the posterior of the parameters of its m absorbers ("slots").
 *  - weights: a sample of model m whose slot 2 .. m holds base index 0 (never drawn), or one above S,
 *    counts as l_i = NaN.  w_i = exp(l_i - max l) over the non-NaN entries; NaN and -inf weigh 0.  No
 *    finite entry, or a maximum of +inf: every output of that (row, model) is NaN and status bit 1 is
 *    set.  T = Sum w_i.  A sample of weight 0 does not exist for anything below.
 *  - slot values: slot 1 of sample i has the parameters of sample i, slot j >= 2 those of sample
 *    base_sample_inds[row][j - 2][i] - 1 (1-based, multi :347, :441): log N = log_nhi_samples[b],
 *    z = min_z + (max_z - min_z) offset_samples[b], each operation rounded on its own.  A NaN min_z or
 *    max_z makes the z outputs (mean_z, std_z, cov, quantiles_z) of the row NaN and sets status bit 2.
 *  - per slot: mean = Sum w v / T; var = Sum w (v - mean)^2 / T about the computed mean, std =
 *    sqrt(var); cov(z, log N) likewise; exceedance[t] = Sum over log N_i >= thresholds[t] of w_i / T.
 *  - per model: effective_samples = T^2 / Sum w^2.
 *  - quantiles: with F(v) = Sum over v_i <= v of w_i, the smallest sample value v* (of a sample of
 *    positive weight) with F(v*) >= p T.  No interpolation: the answer is bitwise one of the slot's
 *    values.  F is summed in a fixed order of its own, so where p T lies within rounding of a step of
 *    F the neighbouring value may be named.
 * Probabilities: 0 .. GPDLA_POSTERIOR_MAX_PROBABILITIES of them, each in (0, 1), strictly increasing.
 * Thresholds: 0 .. GPDLA_POSTERIOR_MAX_THRESHOLDS, not NaN.  Checked before the device is touched.
 *
 * Outputs are [n][num_models][num_models] in (model, slot) order per field -- quantiles with a
 * trailing [num_probabilities], exceedance with a trailing [num_thresholds] -- NaN where slot > model;
 * effective_samples and status are [n][num_models].  Any output pointer may be NULL.
 *
 * Every sum runs in a fixed order without atomics: an output depends on its own row only, is
 * bit-identical from run to run, for any selection and order, and for the host and the resident form
 * of the same table.
 *
 * gpdla_stats_parameter_summaries: host tables.  Row r, model m starts at sample_log_likelihoods +
 * r * row_stride + (m - 1) * num_samples (row_stride >= num_models * num_samples);
 * base_sample_inds is [num_rows][num_models - 1][num_samples], NULL exactly when num_models == 1.
 *
 * gpdla_batch_parameter_summaries: the same kernel on the batch's resident tables after
 * gpdla_batch_process (multi == 0) / gpdla_batch_process_multi (multi != 0: num_models must be the
 * batch's max_dlas); no second sweep, no download of the table.  sub_dla != 0 (multi-DLA batch,
 * num_models 1): the sub-DLA table with log10 of lls_nhi_samples as a one-model, one-slot problem.
 * selection: quasars of the batch, NULL = 0 .. num_selected - 1.
 * ------------------------------------------------------------------------------------------- */
#define GPDLA_POSTERIOR_MAX_MODELS 4
#define GPDLA_POSTERIOR_MAX_PROBABILITIES 8
#define GPDLA_POSTERIOR_MAX_THRESHOLDS 4
#define GPDLA_POSTERIOR_UNUSABLE 1   /* status bit 1 */
#define GPDLA_POSTERIOR_NAN_RANGE 2  /* status bit 2 */
typedef struct {
  int32_t num_models;                /* 1 .. GPDLA_POSTERIOR_MAX_MODELS */
  int32_t num_probabilities;
  double probabilities[GPDLA_POSTERIOR_MAX_PROBABILITIES];
  int32_t num_thresholds;
  double thresholds[GPDLA_POSTERIOR_MAX_THRESHOLDS];
} gpdla_summary_request;
typedef struct {
  double *mean_z, *std_z, *mean_log_nhi, *std_log_nhi, *cov;   /* [n][md][md] */
  double *quantiles_z, *quantiles_log_nhi;                     /* [n][md][md][num_probabilities] */
  double *exceedance;                                          /* [n][md][md][num_thresholds] */
  double *effective_samples;                                   /* [n][md] */
  int32_t *status;                                             /* [n][md] */
} gpdla_parameter_summaries;
int gpdla_stats_parameter_summaries(int64_t num_rows, int64_t num_samples, const double *sample_log_likelihoods,
                                    int64_t row_stride, const uint32_t *base_sample_inds, const double *min_z_dlas,
                                    const double *max_z_dlas, const double *offset_samples,
                                    const double *log_nhi_samples, const gpdla_summary_request *request,
                                    gpdla_parameter_summaries *outputs, int device_id);
int gpdla_batch_parameter_summaries(gpdla_context *ctx, gpdla_batch *batch, int multi, int sub_dla,
                                    const int64_t *selection, int64_t num_selected,
                                    const gpdla_summary_request *request, gpdla_parameter_summaries *outputs);
/* Measuring aid for tools/bench_posteriors.py: the duration of the k_parameter_summaries launch of the
 * calling thread's most recent successful call of either function above, from device events (-1 before
 * the first). */
double gpdla_debug_last_summaries_ms(void);

/* ---------------------------------------------------------------------------------------------
 * Refined absorber posteriors: per-quasar zoom boxes of (z_DLA, log10 N_HI) around the
 * posterior mass of a processed single-DLA batch, re-swept on a shared unit-square point set.  Additive:
 * GPDLA_ABI_VERSION is unchanged.  fp64, k <= 40, single-DLA batches; anything else is
 * GPDLA_ERR_UNSUPPORTED.  Nothing of this exists in the reference.
 *
 * Every operation is rounded on its own; every reduction runs in a fixed order without atomics; a
 * quasar's results depend on that quasar only: bit-identical from run to run and for any selection, order
 * and record grouping.  tests/refine_restatement.py states the same in NumPy.
 *
 * Inputs per selected quasar: its first-pass row l_i, i < S, with z_i = min_z + (max_z - min_z)
 * offset_samples[i] and n_i = log_nhi_samples[i] (log10 of nhi_samples[i], taken by the host, where the
 * samples came without that table); [N_lo, N_hi] = the range of the whole log N table; the request's
 * delta > 0, pad >= 0 and levels L in 1 .. GPDLA_REFINE_MAX_LEVELS; the context's point set (u_j, v_j) in
 * [0, 1)^2, j < S' (S' need not equal S); optionally a gpdla_nhi_prior p_N (NULL: p_N = 1 / (N_hi - N_lo),
 * its logarithm -log(N_hi - N_lo) taken by the host).
 *
 * Unusable rows: quasar status != 0, no finite l_i, a maximum of +inf, a NaN min_z or max_z, or max_z <
 * min_z; at a later level, no finite lambda_j or a maximum of +inf.  Every output of such a row is NaN
 * (boxes of the levels reached before are kept), its refine status has bit 1 (GPDLA_REFINE_UNUSABLE) set,
 * and it is not swept (again).  A quasar outside the last call's selection has status
 * GPDLA_REFINE_NOT_REFINED and NaN outputs.
 *
 * Box of level 1 from (l_i, z_i, n_i) with parent P = (min_z, max_z, N_lo, N_hi) and s = sqrt(S); box of
 * level l + 1 from (lambda_j, z'_j, n'_j) of level l with P = box l and s = sqrt(S'):
 *   A = {i : l_i >= max l - delta} (NaN never qualifies; the maximum skips NaN),
 *   z_lo = max(P.z_lo, min_A z - pad (P.z_hi - P.z_lo) / s),  z_hi = min(P.z_hi, max_A z + pad (P.z_hi - P.z_lo) / s),
 *   n_lo = max(P.n_lo, min_A n - pad (P.n_hi - P.n_lo) / s),  n_hi = min(P.n_hi, max_A n + pad (P.n_hi - P.n_lo) / s).
 * A zero-width box is legal.
 *
 * Samples of level l: z'_j = z_lo + (z_hi - z_lo) u_j, n'_j = n_lo + (n_hi - n_lo) v_j, N'_j = exp10(n'_j),
 * l'_j = the sweep's log-likelihood at (z'_j, N'_j), lambda_j = l'_j + log p_N(n'_j).
 *
 * Refined evidence: with V_l = (z_hi - z_lo) / (max_z - min_z) of box l (1 where max_z == min_z) and
 * W_l = n_hi - n_lo, Z_ref = Sum_{t = 0 .. L} exp(m_t) s_t with
 *   t = 0:           m = max of l_i over i outside box 1,  s = (Sum over i outside box 1 of exp(l_i - m)) / S,
 *   t = 1 .. L - 1:  m = max of lambda_j (level t) over j outside box t + 1,
 *                    s = (V_t W_t) ((Sum over j outside box t + 1 of exp(lambda_j - m)) / S'),
 *   t = L:           m = max lambda_j (level L), s = (V_L W_L) ((Sum over all j of exp(lambda_j - m)) / S'),
 * "outside" meaning z or n strictly beyond an edge and NaN contributing 0.  Every term is shifted by the maximum of
 * the samples it sums, not of its level: on a narrow posterior the level's maximum lies inside the next box,
 * thousands above everything outside it.  A term with nothing outside its box (or -inf only) is m = -inf, s = 0.
 * The terms with s_t > 0 are added in this order as exp(m_t - M) s_t with the one shift M = the largest m_t among
 * them (a term of 0 has no say in the shift), and log_likelihoods_dla_refined = M + log of that sum (-inf where no
 * term is left); log_posteriors_dla_refined adds the batch's log_priors_dla.  The batch's own results and model
 * posteriors are not touched.
 *
 * Refined MAP: the first j of largest lambda_j at level L: MAP_z_dlas_refined = z'_j, MAP_log_nhis_refined
 * = n'_j, MAP_inds_refined = j + 1.
 *
 * gpdla_refine_validate: the checks of a request, a prior (may be NULL) and a point set (num_points == 0
 * with NULL u, v: not checked) that the calls below make before they touch the device.  Needs no GPU.
 * gpdla_context_set_refine_points: copies the point set; u and v finite in [0, 1), 1 <= num_points <= 2^30.
 * gpdla_batch_refine: asynchronous on the context's stream, after gpdla_batch_process of the same
 * spectra.  selection: quasars of the batch (NULL: 0 .. num_selected - 1), duplicates allowed.  Record
 * groups (cfg.record_pool_bytes) are honoured as by the first pass; changing that setting between the
 * two is GPDLA_ERR_INVALID_ARGUMENT.  The tables are allocated on first use and kept across reloads.
 * Resident afterwards: the boxes of every level, the last level's l' and lambda, the scalars above.
 * gpdla_batch_download_refined: rows of the given quasars; boxes is [n][levels of the last call][4] as
 * (z_lo, z_hi, n_lo, n_hi); the two tables are [n][S'].  Any output pointer may be NULL.  results->levels and
 * results->num_points state what the arrays were sized for; a value that differs from the last gpdla_batch_refine's
 * levels / S' is GPDLA_ERR_INVALID_ARGUMENT and nothing is written.
 * gpdla_batch_refined_summaries: gpdla_parameter_summaries (num_models = 1) of the resident lambda table
 * as weights over (z'_j, n'_j) of the last level: same definitions, outputs [n][1][1]...  Refused
 * (GPDLA_ERR_INVALID_ARGUMENT) once gpdla_context_set_refine_points has been called again after the refine.
 * gpdla_batch_refined_posteriors: the model posteriors of the selected quasars with the
 * refined evidence in the place of the first pass's.  For a quasar of refine status 0, with lp_no = the
 * first pass's log_posteriors_no_dla and lp_dla = log_posteriors_dla_refined, the five operations of the
 * first pass, each rounded on its own: mx = max(lp_no, lp_dla), p0 = exp(lp_no - mx), p1 = exp(lp_dla - mx),
 * model_posteriors_refined = (p0, p1) / (p0 + p1), p_no_dlas_refined = the first of the two, p_dlas_refined =
 * 1 - it, refined = 1.  Any other quasar (outside the refine's selection, or unusable) gets the first pass's
 * model_posteriors, p_no_dlas and p_dlas and refined = 0, so the table is complete.  The kernel runs on the
 * context's stream behind the refine; the call returns when the rows are in the caller's arrays.  Legal only
 * after a gpdla_batch_refine of the same spectra (else GPDLA_ERR_INVALID_ARGUMENT, nothing written);
 * selection as for gpdla_batch_download_refined; any output pointer may be NULL.
 * ------------------------------------------------------------------------------------------- */
#define GPDLA_REFINE_MAX_LEVELS 4
#define GPDLA_REFINE_UNUSABLE 1        /* status bit 1 */
#define GPDLA_REFINE_NOT_REFINED (-1)  /* status of a quasar outside the last call's selection */
typedef struct {
  int32_t levels;                    /* 1 .. GPDLA_REFINE_MAX_LEVELS */
  double delta;                      /* > 0: samples within delta of the maximum span the box */
  double pad;                        /* >= 0: in units of (parent width) / sqrt(samples) */
} gpdla_refine_request;
typedef struct {
  int32_t levels;                               /* what the caller sized boxes for: must equal the last call's levels */
  int64_t num_points;                           /* what the caller sized the two tables for: must equal S' */
  double *boxes;                                /* [n][levels][4] */
  double *sample_log_likelihoods_refined;       /* [n][S'] l' of the last level */
  double *sample_log_posteriors_refined;        /* [n][S'] lambda of the last level */
  double *log_likelihoods_dla_refined, *log_posteriors_dla_refined;        /* [n] */
  double *MAP_z_dlas_refined, *MAP_log_nhis_refined, *MAP_inds_refined;    /* [n] */
  int32_t *status;                              /* [n] */
} gpdla_refined_results;
int gpdla_refine_validate(const gpdla_refine_request *request, const gpdla_nhi_prior *prior, int64_t num_points,
                          const double *u, const double *v);
int gpdla_context_set_refine_points(gpdla_context *ctx, int64_t num_points, const double *u, const double *v);
int gpdla_batch_refine(gpdla_context *ctx, gpdla_batch *batch, const int64_t *selection, int64_t num_selected,
                       const gpdla_refine_request *request, const gpdla_nhi_prior *prior);
int gpdla_batch_download_refined(gpdla_context *ctx, gpdla_batch *batch, const int64_t *selection,
                                 int64_t num_selected, gpdla_refined_results *results);
int gpdla_batch_refined_summaries(gpdla_context *ctx, gpdla_batch *batch, const int64_t *selection,
                                  int64_t num_selected, const gpdla_summary_request *request,
                                  gpdla_parameter_summaries *outputs);
typedef struct {
  double *model_posteriors_refined;             /* [n][2] (no DLA, DLA) */
  double *p_no_dlas_refined, *p_dlas_refined;   /* [n] */
  int32_t *refined;                             /* [n] 1: from the refined evidence, 0: the first pass's */
} gpdla_refined_posteriors;
int gpdla_batch_refined_posteriors(gpdla_context *ctx, gpdla_batch *batch, const int64_t *selection,
                                   int64_t num_selected, gpdla_refined_posteriors *out);
/* Measuring aid for tools/bench_refine.py: device time of the calling thread's most recent gpdla_batch_refine
 * made with the context's timing on (all groups and levels; -1 before the first). */
double gpdla_debug_last_refine_ms(void);

/* ---------------------------------------------------------------------------------------------
 * A batch conditioned on fixed absorbers.  Additive: GPDLA_ABI_VERSION is unchanged.
 * Single-DLA batches (uploaded without log_priors_lls), fp64, k <= 40; anything else is
 * GPDLA_ERR_UNSUPPORTED.  Nothing of this exists in the reference; the identity it rests on is the
 * reference's own k-DLA likelihood (multi :342-351), which multiplies mu, M and omega by the product of all k
 * profiles.  With k - 1 absorbers held fixed, their product A is a vector per quasar; on the rows mu A, M A,
 * omega2 A^2 the single-DLA sweep is the k-DLA likelihood as a function of the remaining absorber alone.
 *
 * gpdla_fixed_absorbers_validate: the checks that gpdla_batch_set_fixed_absorbers makes of its lists, in
 * this order; the first that fails is GPDLA_ERR_INVALID_ARGUMENT, its message names the field and the quasar,
 * and nothing is written.  offsets [num_quasars + 1] into z_dlas / log_nhis (log10 N_HI), non-decreasing, at
 * most GPDLA_MAX_FIXED_ABSORBERS per quasar; min_z_separation finite and >= 0; every z_dla and log_nhi finite;
 * no two fixed absorbers of one quasar closer than min_z_separation (larger - smaller < min_z_separation).
 * Needs no GPU.
 *
 * gpdla_batch_set_fixed_absorbers: copies the lists (N = pow(10, log_nhi), taken by the host) and makes the
 * batch a conditioned one.  meanflux_rows = 1: the rows are prepared as the multi-DLA driver prepares them
 * (Lyman-series noise scaling and mean-flux suppression by the context's num_forest_lines, prev_tau_0,
 * prev_beta), so that the sweep is the multi-DLA model's likelihood; 0: the rows of process_qsos.m.
 * gpdla_batch_clear_fixed_absorbers makes it an ordinary batch again.  Either marks the batch unprocessed and
 * not refined; gpdla_batch_reload clears.
 *
 * gpdla_batch_process on a conditioned batch: k_prepare, then per quasar with at least one fixed absorber
 * and status 0
 *   A_u = the product, in list order, of the instrument-broadened Lyman-series profiles (the context's
 *         num_lines) of its fixed absorbers on its unmasked-range grid: what gpdla_batch_model_spectra
 *         returns as map_absorption for the same list, bit for bit,
 *   mu_u <- mu_u A_u,  omega2_u <- omega2_u (A_u A_u),  M_uc <- M_uc A_u  (c < k), each rounded once;
 * y and nu are not touched, a masked (neutral) row stays neutral.  Records and sweep as for any batch.  Then
 * the separation rule of multi :386-392 for one free absorber among fixed ones: sample i, whose own
 * z_i = min_z + (max_z - min_z) offset_samples[i], gets sample_log_likelihoods_dla = -inf where
 * max(z_i, z_f) - min(z_i, z_f) < min_z_separation for any fixed z_f.  -inf, not the reference's NaN: zero
 * likelihood inside the separation (the refine contract's "NaN contributes 0"), which keeps the mean over S
 * of log_likelihoods_dla defined; the reference's nanmean would renormalise by the surviving samples instead.
 * A quasar without fixed absorbers is not touched: its results equal an unconditioned batch's bit for bit.
 *
 * gpdla_batch_refine on a conditioned batch: as above; the records are rebuilt from the conditioned rows,
 * and the same rule runs on l' of each level, z'_j = z_lo + (z_hi - z_lo) u_j, before lambda is formed.
 *
 * What the results mean: log_likelihoods_no_dla is the likelihood of the fixed absorbers alone; every other
 * result (evidences, posteriors, MAPs, the refined tables, their summaries) is about ONE MORE absorber given
 * them.  gpdla_batch_download, gpdla_batch_download_refined, gpdla_batch_refined_summaries,
 * gpdla_batch_refined_posteriors and gpdla_batch_parameter_summaries serve such a batch as they are.  The
 * entries that prepare the batch's rows again (gpdla_batch_model_spectra, gpdla_batch_unmasked_counts,
 * gpdla_batch_draw_mocks, gpdla_debug_prepared_rows) refuse it with GPDLA_ERR_UNSUPPORTED.
 *
 * gpdla_debug_conditioned_rows (test hook): k_prepare and, on a conditioned batch, the conditioning alone;
 * then the rows (y, mu, omega2, nu) [n][4] and, if M_out is not NULL, the M rows [n][k] of one quasar on its
 * unmasked-range grid, n = min(n_u, capacity_rows).  meanflux_rows chooses the preparation of an
 * UNconditioned batch; a conditioned one uses its own.
 * ------------------------------------------------------------------------------------------- */
#define GPDLA_MAX_FIXED_ABSORBERS 8
int gpdla_fixed_absorbers_validate(int64_t num_quasars, const int64_t *offsets, const double *z_dlas,
                                   const double *log_nhis, double min_z_separation);
int gpdla_batch_set_fixed_absorbers(gpdla_context *ctx, gpdla_batch *batch, const int64_t *offsets,
                                    const double *z_dlas, const double *log_nhis, double min_z_separation,
                                    int32_t meanflux_rows);
int gpdla_batch_clear_fixed_absorbers(gpdla_context *ctx, gpdla_batch *batch);
int gpdla_debug_conditioned_rows(gpdla_context *ctx, gpdla_batch *batch, int32_t meanflux_rows, int64_t quasar,
                                 double *rows_out, double *M_out, int64_t capacity_rows, int64_t *num_rows_out);

/* ---------------------------------------------------------------------------------------------
 * Posterior maps of (z_DLA, log10 N_HI): highest posterior density (HPD) regions per (row, model, slot),
 * and the absorber intensity averaged over the models.  Additive: GPDLA_ABI_VERSION is
 * unchanged.  Nothing of this exists in the reference; tests/posterior_maps_restatement.py states the same
 * in NumPy.  Every operation is rounded on its own.
 *
 * Per row r, model m (1 .. num_models <= GPDLA_POSTERIOR_MAX_MODELS) and slot j <= m:
 *  - weights: exactly those of the parameter summaries above: the base-index-0 and above-S rule, w_i =
 *    exp(l_i - max l), NaN and -inf weighing 0, T = Sum w_i summed as there.  No finite entry, or a maximum
 *    of +inf: every output of the (row, model) is NaN (-1 for the integer outputs) and status bit 1
 *    (GPDLA_MAPS_UNUSABLE) is set.  A sample of weight 0 does not exist for anything below.
 *  - slot values: exactly those of the parameter summaries: z = min_z + (max_z - min_z) offset_samples[b],
 *    log N = log_nhi_samples[b], or n_lo + (n_hi - n_lo) v[b] for the refined tables.  (A NaN min_z or max_z
 *    makes every z NaN: all of the row's mass is outside.)
 *  - grid: the row's (gz_lo, gz_hi, gn_lo, gn_hi) and the request's counts nz, nn, each 1 ..
 *    GPDLA_MAPS_MAX_SIDE.  Per axis (lo, hi, n): edge e_c = lo + (hi - lo) * (c / n) for c < n, c / n a double
 *    division, and e_n = hi itself.  The cell of v is the largest c with e_c <= v for lo <= v < hi; v == hi
 *    is in cell n - 1; v outside [lo, hi], or NaN, is "outside".  Cells are lower-closed, the last closed.
 *    A non-finite grid entry, hi <= lo on either axis, or a width hi - lo that overflows: every map output
 *    of the row is NaN (-1), the row's intensity and expected_absorbers included, and status bit 4
 *    (GPDLA_MAPS_BAD_GRID) is set.
 *  - mass[r][m][j][cz][cn] = (Sum over the cell's samples of w_i, added in sample order) / T;
 *    outside[r][m][j] = the same over the samples with either coordinate outside.
 *  - ranking: the cells of positive mass by mass descending, ties by flat index cz * nn + cn ascending;
 *    C_k = C_(k-1) + mass_(k), accumulated one after the other in rank order, C_0 = 0.
 *  - hpd_level[cell] = C at the cell's rank, NaN for a cell of mass 0: the smallest credible mass whose
 *    region holds the cell.  mode = the flat index of rank 1 (-1 when no cell has mass).  Per requested
 *    credible mass p (0 .. GPDLA_MAPS_MAX_LEVELS of them, each in (0, 1), strictly increasing): hpd_cells[p]
 *    = the smallest k with C_k >= p, hpd_threshold[p] = mass_(k): the region is {cell : mass >= threshold},
 *    cut by index among equal masses.  If no k reaches p (too much mass outside), k is the number of
 *    positive cells (threshold NaN when there is none) and status bit 8 (GPDLA_MAPS_SHORT) is set.
 *  - intensity, when model weights are given: a model of weight exactly 0 is skipped, unusable or not;
 *    s_m = mass[r][m][1][cell] + ... + mass[r][m][m][cell] in slot order from 0; intensity[r][cz][cn] = the
 *    sum of model_weights[r][m] * s_m over the remaining models in model order from 0;
 *    expected_absorbers[r] = the sum of the row's intensity in flat-index order from 0.  A NaN or negative
 *    weight, or a positive weight on an unusable model, makes both NaN and sets status bit 16
 *    (GPDLA_MAPS_BAD_WEIGHTS) in every model's status of the row (a bad grid shows as bit 4 alone).
 * Every sum runs in the stated order without atomics of any kind: an output depends on its own row only and
 * is bit-identical from run to run, for any selection, order and launch grouping, and for the host and the
 * resident form of the same table.
 *
 * Outputs are [n][num_models][num_models] in (model, slot) order per field, NaN / -1 where slot > model:
 * mass and hpd_level with a trailing [nz][nn], hpd_cells and hpd_threshold with a trailing [num_levels];
 * intensity is [n][nz][nn], expected_absorbers [n], status [n][num_models] (the OR over the model's slots).
 * Any output pointer may be NULL; with mass and hpd_level NULL no per-cell array of a slot leaves the
 * device.  intensity / expected_absorbers without weights are GPDLA_ERR_INVALID_ARGUMENT.
 *
 * Every entry checks its request (counts, credible masses, the sample tables' size and finiteness, the
 * base index range) before the device is touched and names the offending field.
 * gpdla_stats_posterior_maps: host tables, the arguments of gpdla_stats_parameter_summaries, the four grid
 * arrays [num_rows] and model_weights [num_rows][num_models] or NULL.
 * gpdla_batch_posterior_maps: the resident tables as gpdla_batch_parameter_summaries reads them (multi,
 * sub_dla, selection).  The four grid arrays [num_selected] come together or are all NULL: then z is the
 * quasar's search range and log N the range of the sample table in use.  model_weights NULL and
 * request->mix != 0: the resident model posteriors of DLA(1 .. num_models) (p_lls for the sub-DLA table,
 * p_dla for a single-DLA batch).
 * gpdla_batch_refined_posterior_maps: the last refine level, as gpdla_batch_refined_summaries reads it
 * (num_models = 1); the default grid is the quasar's last box, the default weight the first pass's p_dla.
 * It serves a conditioned batch as it is.
 * gpdla_posterior_maps_rows_per_launch: the rows one launch group takes: the group's maps
 * ([rows][num_models][num_models][nz][nn] doubles) stay within 256 MiB of device memory; 0 for counts out
 * of range.  gpdla_debug_last_maps_ms (kernel 0: k_posterior_maps, 1: k_posterior_maps_mix, -1 where it
 * did not run) and gpdla_debug_last_maps_launches: device time summed over the groups, and the number of
 * groups, of the calling thread's most recent successful call (tools/bench_posterior_maps.py).
 * ------------------------------------------------------------------------------------------- */
#define GPDLA_MAPS_MAX_SIDE 64
#define GPDLA_MAPS_MAX_LEVELS 8
#define GPDLA_MAPS_UNUSABLE 1      /* status bit 1 */
#define GPDLA_MAPS_BAD_GRID 4      /* status bit 4 */
#define GPDLA_MAPS_SHORT 8         /* status bit 8 */
#define GPDLA_MAPS_BAD_WEIGHTS 16  /* status bit 16 */
typedef struct {
  int32_t num_models;                /* 1 .. GPDLA_POSTERIOR_MAX_MODELS */
  int32_t nz, nn;                    /* cells per axis, 1 .. GPDLA_MAPS_MAX_SIDE each */
  int32_t num_levels;
  double levels[GPDLA_MAPS_MAX_LEVELS];
  int32_t mix;                       /* batch entries: with NULL model_weights, mix by the resident posteriors */
} gpdla_posterior_maps_request;
typedef struct {
  double *mass, *hpd_level;          /* [n][md][md][nz][nn] */
  double *outside;                   /* [n][md][md] */
  int32_t *mode;                     /* [n][md][md] */
  int32_t *hpd_cells;                /* [n][md][md][num_levels] */
  double *hpd_threshold;             /* [n][md][md][num_levels] */
  double *intensity;                 /* [n][nz][nn] */
  double *expected_absorbers;        /* [n] */
  int32_t *status;                   /* [n][md] */
} gpdla_posterior_maps;
int gpdla_stats_posterior_maps(int64_t num_rows, int64_t num_samples, const double *sample_log_likelihoods,
                               int64_t row_stride, const uint32_t *base_sample_inds, const double *min_z_dlas,
                               const double *max_z_dlas, const double *offset_samples, const double *log_nhi_samples,
                               const double *grid_z_lo, const double *grid_z_hi, const double *grid_n_lo,
                               const double *grid_n_hi, const double *model_weights,
                               const gpdla_posterior_maps_request *request, gpdla_posterior_maps *outputs, int device_id);
int gpdla_batch_posterior_maps(gpdla_context *ctx, gpdla_batch *batch, int multi, int sub_dla, const int64_t *selection,
                               int64_t num_selected, const double *grid_z_lo, const double *grid_z_hi,
                               const double *grid_n_lo, const double *grid_n_hi, const double *model_weights,
                               const gpdla_posterior_maps_request *request, gpdla_posterior_maps *outputs);
int gpdla_batch_refined_posterior_maps(gpdla_context *ctx, gpdla_batch *batch, const int64_t *selection,
                                       int64_t num_selected, const double *grid_z_lo, const double *grid_z_hi,
                                       const double *grid_n_lo, const double *grid_n_hi, const double *model_weights,
                                       const gpdla_posterior_maps_request *request, gpdla_posterior_maps *outputs);
int64_t gpdla_posterior_maps_rows_per_launch(int num_models, int nz, int nn);
double gpdla_debug_last_maps_ms(int kernel);
int64_t gpdla_debug_last_maps_launches(void);

/* ---------------------------------------------------------------------------------------------
 * Marginal continuum: the GP posterior mean and variance of the low-rank continuum over the sample tables
 * and over the models.  Additive: GPDLA_ABI_VERSION is unchanged.  fp64 throughout;
 * tests/marginal_continuum_restatement.py states the same in NumPy.
 *
 * Quasar q has the prepared rows (y, mu, M, omega2, nu) of the preparation kernel (meanflux != 0: the
 * suppressed rows).  Sample i has the broadened profile a_i on the quasar's grid, exactly the profile of
 * mean_absorption above (z_i, N_i from nhi_samples, or lls_nhi_samples for the sub-DLA table).  Per sample
 *   d_i = a_i^2 omega2 + nu,  B_i = I + M' diag(a_i^2 / d_i) M,  v_i = M' (a_i (y - a_i mu) / d_i),
 *   c_i = B_i^-1 v_i,  Sigma_i = B_i^-1:
 * the posterior mean and covariance of the coefficients c ~ N(0, I) given sample i.  The weights w_i are
 * those of mean_absorption (exp(l_i - max l) / Sum, NaN -> 0).  One sampled component:
 *   cbar = Sum w_i c_i,  W = Sum w_i Sigma_i (within),  V = Sum w_i c_i c_i' - cbar cbar' (between).
 * The null component is a = 1: c_0, Sigma_0, no spread.  The mixture runs over (null, sub-DLA table, DLA
 * table) with the per-quasar model_weights p, each row non-negative, finite, of positive sum and normalised
 * by its sum (NULL: (0, 0, 1) for every quasar):
 *   c = Sum p_m cbar_m,  W = Sum p_m W_m,  V = Sum p_m (V_m + cbar_m cbar_m') - c c'.
 * A component of weight exactly 0 is not evaluated; a sample of weight exactly 0 is skipped (its B_i is never
 * factorised).  Per pixel p of the unmasked-range grid, m_p interpolated (and suppressed) as for continuum:
 *   continuum_mean = mu_p + m_p' c,  continuum_var = m_p' (W + V) m_p,  continuum_var_between = m_p' V m_p.
 * The pixel-diagonal omega term predicts nothing at a pixel that was not measured and is left out, as for
 * continuum: continuum_var is the variance of the LOW-RANK part of the GP.
 * coef_mean [num_selected][k] = c; coef_cov_within, coef_cov_between [num_selected][k (k + 1) / 2] = W, V as
 * packed lower triangles stored row by row.  sample_coefficients [num_selected][S][k] (request flag; the
 * model weights must reach exactly one table): c_i per sample, in sample order, NaN rows for samples of weight 0.
 * status: the quasar's sweep status (1, 3: NaN rows); 4 = a B_i of positive weight, or B_0, is not positive
 * definite (NaN rows).  A table of positive model weight whose row has no weights (all NaN, all -inf, a +inf)
 * gives NaN rows and status 0.  For a multi-DLA batch the resident tables are model DLA(1) and the sub-DLA
 * table.  A conditioned batch is refused.  Sums run in a fixed order without atomics: outputs are bit-identical
 * for any selection order and launch grouping and for the resident and the host form of a table.
 *
 * THE REFINED SOURCE (GPDLA_SPECTRA_WEIGHTS_REFINED): the DLA component is its definition above with
 * (S, offset_i, N_i, l, min_z_dla, max_z_dla) replaced by (S', u, N', lambda, z_lo, z_hi) of the batch's refine pass, as
 * defined for mean_absorption under "THE REFINED SOURCE": the samples are the S' refine points mapped through the quasar's
 * last box, the weights those of its resident lambda row.  Everything else is unchanged -- the profile, the broadening,
 * d_i, B_i, c_i, Sigma_i, the reductions and the mixture; the null component is unchanged; the sub-DLA component keeps the
 * first-pass sub-DLA table and its own S samples, so a mixture may hold components of different sample counts.  Posterior
 * mass outside the last box is ignored (the convention of the refined parameter summaries).  sample_coefficients is
 * [num_selected][S'][k] when the one component is the refined DLA table.  GPDLA_ERR_INVALID_ARGUMENT when some row weighs the
 * DLA component and the batch has not been refined, or the context's refine points changed since the refine.  A selected
 * quasar whose DLA component carries weight and whose refine status is not 0 (outside the refine's selection, or unusable)
 * gets NaN rows and status GPDLA_SPECTRA_NOT_REFINED; where the DLA component weighs exactly 0 the quasar is evaluated as
 * before.  The bit-identity promise holds.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t num_selected;
  const int64_t *selection;          /* [num_selected] quasars of the batch; NULL = 0 .. num_selected-1 */
  int32_t weights_source;            /* GPDLA_SPECTRA_WEIGHTS_RESIDENT, _HOST or _REFINED (_NONE: null component only) */
  const double *sample_log_likelihoods_dla; /* [num_selected][S], _HOST, where a row weighs the DLA table */
  const double *sample_log_likelihoods_lls; /* [num_selected][S], _HOST, where a row weighs the sub-DLA table */
  const double *model_weights;       /* [num_selected][3] (null, sub-DLA, DLA), or NULL = (0, 0, 1) */
  int32_t meanflux;                  /* != 0: prepared rows of the mean-flux model (multi :245-293) */
  int32_t sample_coefficients;       /* != 0: fill sample_coefficients */
  int64_t capacity;                  /* entries of each per-pixel output array */
} gpdla_marginal_continuum_request;
typedef struct {
  int64_t *offsets;                  /* [num_selected + 1]; required */
  double *continuum_mean, *continuum_var, *continuum_var_between; /* per pixel; any may be NULL */
  double *coef_mean;                 /* [num_selected][k] or NULL */
  double *coef_cov_within, *coef_cov_between; /* [num_selected][k (k + 1) / 2] or NULL */
  double *sample_coefficients;       /* [num_selected][S][k] or NULL */
  int32_t *status;                   /* [num_selected] or NULL */
} gpdla_marginal_continuum;
/* The checks gpdla_batch_marginal_continuum makes before its first device call: a selection index outside the
 * batch, a negative, NaN or infinite model weight or a row without a positive sum, a sampled component
 * without a weights source (or a host source without that table), the sub-DLA table without lls_nhi_samples,
 * sample_coefficients with both tables or none.  Returns GPDLA_OK or GPDLA_ERR_INVALID_ARGUMENT.  Needs no GPU. */
int gpdla_marginal_continuum_validate(const gpdla_marginal_continuum_request *request, int64_t num_quasars,
                                      int64_t num_samples, int has_lls_nhi_samples);
/* With gpdla_context_set_timing enabled, gpdla_context_last_sweep_ms reports the launch groups of the call: per
 * group the staging of a host table's slice, k_spectra_weights, k_mc_contract, k_mc_solve and k_mc_finish. */
int gpdla_batch_marginal_continuum(gpdla_context *ctx, gpdla_batch *batch, const gpdla_marginal_continuum_request *request,
                                   gpdla_marginal_continuum *out);

/* ---------------------------------------------------------------------------------------------
 * Posterior predictive flux: per pixel, the mean and variance of the model flux -- absorption times continuum --
 * over the sample tables and over the models.  Additive: GPDLA_ABI_VERSION is unchanged.  fp64
 * throughout; tests/predictive_flux_restatement.py states the same in NumPy.
 *
 * Quasar q, component m of (null, sub-DLA table, DLA table) and sample i of weight w_i > 0 are exactly those of
 * gpdla_batch_marginal_continuum above: the same prepared rows (y, mu, M, omega2, nu; meanflux != 0: the
 * suppressed rows), the same broadened profile a_i on the quasar's grid (z_i, N_i from nhi_samples, or
 * lls_nhi_samples for the sub-DLA table), the same weights w_i (exp(l_i - max l) / Sum, NaN -> 0), and per sample
 *   d_i = a_i^2 omega2 + nu,  B_i = I + M' diag(a_i^2 / d_i) M,  v_i = M' (a_i (y - a_i mu) / d_i),
 *   c_i = B_i^-1 v_i,  Sigma_i = B_i^-1,
 * the posterior mean and covariance of the coefficients c ~ N(0, I) given sample i.  The model weights p_m are
 * per quasar, each row non-negative, finite, of positive sum and normalised by its sum (NULL: (0, 0, 1)).
 * For EVERY pixel p of the unmasked-range grid, mu_p and m_p are interpolated (and suppressed under meanflux)
 * as for continuum_mean; a masked pixel is treated like a kept one.  Per sample
 *   t_ip = mu_p + m_p' c_i  (the continuum given sample i),  s_ip = m_p' Sigma_i m_p  (its variance),
 *   f_ip = a_ip t_ip        (the model flux given sample i).
 * The null component has a = 1, c_0, Sigma_0 and one "sample" of weight 1.  Per component
 *   F1 = Sum w_i f_ip,  F2 = Sum w_i f_ip^2,  FW = Sum w_i a_ip^2 s_ip,  FD = Sum w_i (a_ip^2 omega2_p + nu_p),
 * and the mixture over the models, in the order (null, sub-DLA, DLA):
 *   flux_mean        = Sum p_m F1_m
 *   flux_var_within  = Sum p_m FW_m                             (the GP's own spread, given the absorber)
 *   flux_var_between = max(Sum p_m F2_m - flux_mean^2, 0)       (the spread over absorbers and models)
 *   flux_var         = flux_var_within + flux_var_between
 *   noise_var        = Sum p_m FD_m on kept pixels, NaN on masked ones (they have no omega2 and nu).
 * E[a t] is not E[a] E[t]: c_i moves with the absorber, which is why this is not a product of mean_absorption
 * and continuum_mean.  Sum w f^2 - (Sum w f)^2 is evaluated unfused, so a one-hot weight row gives a
 * flux_var_between of exactly 0.
 * As for continuum and continuum_var, flux_var is the variance of the LOW-RANK, NOISE-FREE model flux: the
 * pixel-diagonal omega term and the measurement noise are left out of it.  flux_var + noise_var is the variance
 * of a REPLICATE observation of the pixel: a new draw of the pixel-diagonal term and of the noise under the same
 * posterior.  These are in-sample moments (the pixel's own flux is in the data the posterior was formed from),
 * not leave-one-out ones.
 * A component of weight exactly 0 is not evaluated; a sample of weight exactly 0 is never touched (its B_i is
 * never factorised, its column density may be NaN).  status: the quasar's sweep status (1, 3: NaN rows); 4 = a
 * B_i of positive weight, or B_0, is not positive definite (NaN rows).  A table of positive model weight whose
 * row has no weights (all NaN, all -inf, a +inf) gives NaN rows and status 0.  For a multi-DLA batch the
 * resident tables are model DLA(1) and the sub-DLA table.  A conditioned batch is refused.  Sums run in a fixed
 * order without atomics: outputs are bit-identical for any selection order and launch grouping and for the
 * resident and the host form of a table.
 *
 * THE REFINED SOURCE (GPDLA_SPECTRA_WEIGHTS_REFINED): exactly as for gpdla_batch_marginal_continuum above --
 * the DLA component runs on the S' refine points mapped through the quasar's last box, weighted by its resident lambda row;
 * the null and the sub-DLA component are unchanged; mass outside the last box is ignored; the same refusals and the same
 * NaN rows with status GPDLA_SPECTRA_NOT_REFINED.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t num_selected;
  const int64_t *selection;          /* [num_selected] quasars of the batch; NULL = 0 .. num_selected-1 */
  int32_t weights_source;            /* GPDLA_SPECTRA_WEIGHTS_RESIDENT, _HOST or _REFINED (_NONE: null component only) */
  const double *sample_log_likelihoods_dla; /* [num_selected][S], _HOST, where a row weighs the DLA table */
  const double *sample_log_likelihoods_lls; /* [num_selected][S], _HOST, where a row weighs the sub-DLA table */
  const double *model_weights;       /* [num_selected][3] (null, sub-DLA, DLA), or NULL = (0, 0, 1) */
  int32_t meanflux;                  /* != 0: prepared rows of the mean-flux model (multi :245-293) */
  int64_t capacity;                  /* entries of each per-pixel output array */
} gpdla_predictive_flux_request;
typedef struct {
  int64_t *offsets;                  /* [num_selected + 1]; required */
  double *flux_mean, *flux_var, *flux_var_within, *flux_var_between, *noise_var; /* per pixel; any may be NULL */
  int32_t *status;                   /* [num_selected] or NULL */
} gpdla_predictive_flux;
/* The checks gpdla_batch_predictive_flux makes before its first device call, which are those of
 * gpdla_marginal_continuum_validate: a selection index outside the batch, a negative, NaN or infinite model
 * weight or a row without a positive sum, a sampled component without a weights source (or a host source
 * without that table), the sub-DLA table without lls_nhi_samples.  Returns GPDLA_OK or
 * GPDLA_ERR_INVALID_ARGUMENT.  Needs no GPU. */
int gpdla_predictive_flux_validate(const gpdla_predictive_flux_request *request, int64_t num_quasars,
                                   int64_t num_samples, int has_lls_nhi_samples);
/* With gpdla_context_set_timing enabled, gpdla_context_last_sweep_ms reports the launch groups of the call: per
 * group the staging of a host table's slice, k_spectra_weights, k_mc_contract, k_pf_solve, k_pf_live, k_pf_pixels and
 * k_pf_finish. */
int gpdla_batch_predictive_flux(gpdla_context *ctx, gpdla_batch *batch, const gpdla_predictive_flux_request *request,
                                gpdla_predictive_flux *out);

/* ---------------------------------------------------------------------------------------------
 * Marginal continuum and posterior predictive flux over ALL models of a multi-DLA run.
 * Additive: GPDLA_ABI_VERSION is unchanged.  fp64 throughout; tests/marginal_continuum_multi_restatement.py and
 * tests/predictive_flux_multi_restatement.py state the same in NumPy.
 *
 * Every definition of gpdla_batch_marginal_continuum and gpdla_batch_predictive_flux above holds unchanged: the
 * prepared rows, d_i, B_i, v_i, c_i, Sigma_i; cbar, W, V; per pixel t_ip, s_ip, f_ip, F1, F2, FW, FD; the
 * pixel-diagonal term left out; masked pixels treated as kept ones except for noise_var.  Two things change.
 *
 * 1. Components, in this order: null; the sub-DLA table; DLA(1), .., DLA(max_dlas).  For model DLA(n), sample i:
 *   profile  a_i = A_{n,i}(p) = Prod_{j=1..n} c_{s_j(i)}(p) of gpdla_batch_model_spectra_multi, word for word: the
 *            slots s_1(i) = i, s_j(i) = base_sample_inds[q][j-2][i] - 1, the product of the BROADENED profiles
 *            (z, N of nhi_samples) in slot order;
 *   weight   that entry's: w_i = exp(l_i - max l) / Sum from row sample_log_likelihoods_dla[q][n-1][.], a NaN l_i
 *            weighs 0, a sample one of whose slots j >= 2 has base index 0 ("never drawn") is read as NaN.
 *   The sub-DLA table and DLA(1) are the two sampled components of the entries above, bit for bit.
 * 2. Model weights: model_weights [num_selected][2 + max_dlas] in the order (P_null, P_lls, P_1 .. P_md), or NULL: the
 *   batch's resident model_posteriors (resident tables only).  Each row is normalised by its sum; the sums over the
 *   models run in component order.  A row with a negative or infinite entry, or without a positive finite sum, is
 *   refused.  A row with a NaN entry is NOT refused (the reference's early exit leaves whole model_posteriors rows
 *   NaN): that quasar gets NaN rows and GPDLA_SPECTRA_AVERAGE_UNDEFINED in its status.
 *
 * A component of weight exactly 0 is not evaluated; a sample of weight exactly 0 is never touched (its column
 * density may be NaN).  status: the quasar's sweep status (1, 3: NaN rows); 4 = a B_i of positive weight, or B_0, is
 * not positive definite (NaN rows); GPDLA_SPECTRA_AVERAGE_UNDEFINED as above.  A component of positive weight whose
 * weight row has no weights (all NaN, all -inf, a +inf, every sample consuming a base index of 0) gives NaN rows
 * and status 0, and is named in model_flags[s]: bit n-1 for DLA(n), GPDLA_SPECTRA_MULTI_FLAG_LLS for the sub-DLA
 * table.  A component the quasar does not weigh is never flagged.  A conditioned batch is refused.
 * sample_coefficients are not offered.
 *
 * Sums run in a fixed order without atomics (samples in list / index order, waves in wave order, chunks in chunk
 * order, components in component order): outputs are bit-identical for any selection order and launch grouping
 * and for the resident and the host form of the same tables.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t num_selected;
  const int64_t *selection;          /* [num_selected] quasars of the batch; NULL = 0 .. num_selected-1 */
  int32_t max_dlas;                  /* models of the tables: 1 .. GPDLA_POSTERIOR_MAX_MODELS */
  int32_t tables_source;             /* GPDLA_SPECTRA_WEIGHTS_RESIDENT (after gpdla_batch_process_multi) or _HOST */
  const double *sample_log_likelihoods_dla;  /* host: [num_selected][max_dlas][S], where a row weighs a DLA(n) */
  const uint32_t *base_sample_inds;          /* host: [num_selected][max_dlas-1][S], 1-based, 0 = never drawn,
                                                where a row weighs a DLA(n >= 2) */
  const double *sample_log_likelihoods_lls;  /* host: [num_selected][S], where a row weighs the sub-DLA table */
  const double *model_weights;       /* host [num_selected][2 + max_dlas], or NULL: the resident model_posteriors
                                        (refused for host tables) */
  int32_t meanflux;                  /* != 0: prepared rows of the mean-flux model */
  int64_t capacity;                  /* entries of each per-pixel output array */
} gpdla_marginal_continuum_multi_request;
typedef struct {
  int64_t *offsets;                  /* [num_selected + 1]; required */
  double *continuum_mean, *continuum_var, *continuum_var_between; /* per pixel; any may be NULL */
  double *coef_mean;                 /* [num_selected][k] or NULL */
  double *coef_cov_within, *coef_cov_between; /* [num_selected][k (k + 1) / 2] or NULL */
  int32_t *status;                   /* [num_selected] or NULL */
  uint32_t *model_flags;             /* [num_selected] or NULL */
} gpdla_marginal_continuum_multi;
typedef struct {
  int64_t num_selected;
  const int64_t *selection;
  int32_t max_dlas;
  int32_t tables_source;
  const double *sample_log_likelihoods_dla;
  const uint32_t *base_sample_inds;
  const double *sample_log_likelihoods_lls;
  const double *model_weights;
  int32_t meanflux;
  int64_t capacity;
} gpdla_predictive_flux_multi_request; /* the fields of gpdla_marginal_continuum_multi_request */
typedef struct {
  int64_t *offsets;                  /* [num_selected + 1]; required */
  double *flux_mean, *flux_var, *flux_var_within, *flux_var_between, *noise_var; /* per pixel; any may be NULL */
  int32_t *status;                   /* [num_selected] or NULL */
  uint32_t *model_flags;             /* [num_selected] or NULL */
} gpdla_predictive_flux_multi;
/* The checks the two entries make before their first device call, for a batch of num_quasars quasars uploaded for
 * batch_max_dlas models (0: a single-DLA batch) that has (batch_processed != 0) or has not run
 * gpdla_batch_process_multi: max_dlas outside 1 .. GPDLA_POSTERIOR_MAX_MODELS, a selection index outside the batch,
 * a resident source on a single-DLA batch, on a batch of another max_dlas or on one that has not been processed,
 * host tables without model_weights, a host table that a weighted component needs and that is missing, a host base
 * index above num_samples, a negative or infinite model weight or a row (without a NaN) without a positive finite
 * sum, no lls_nhi_samples while the sub-DLA column carries weight (without model_weights: always).  Return GPDLA_OK
 * or GPDLA_ERR_INVALID_ARGUMENT.  Need no GPU. */
int gpdla_marginal_continuum_multi_validate(const gpdla_marginal_continuum_multi_request *request, int64_t num_quasars,
                                            int64_t num_samples, int has_lls_nhi_samples, int batch_max_dlas,
                                            int batch_processed);
int gpdla_predictive_flux_multi_validate(const gpdla_predictive_flux_multi_request *request, int64_t num_quasars,
                                         int64_t num_samples, int has_lls_nhi_samples, int batch_max_dlas,
                                         int batch_processed);
/* The selected quasars are taken in groups whose scratch rows fit 512 MiB; host tables are staged a group at a time;
 * results do not depend on the grouping.  With gpdla_context_set_timing enabled, gpdla_context_last_sweep_ms reports
 * the kernels of the call (weights, contract, solve, live list, pixels, finish). */
int gpdla_batch_marginal_continuum_multi(gpdla_context *ctx, gpdla_batch *batch,
                                         const gpdla_marginal_continuum_multi_request *request,
                                         gpdla_marginal_continuum_multi *out);
int gpdla_batch_predictive_flux_multi(gpdla_context *ctx, gpdla_batch *batch,
                                      const gpdla_predictive_flux_multi_request *request,
                                      gpdla_predictive_flux_multi *out);

/* ---------------------------------------------------------------------------------------------
 * Absorption distribution: per pixel, the DISTRIBUTION of the absorption over the sample tables and over the models
 *  -- the posterior probability that the transmission is at or below a threshold (forest masks), the
 * support, a histogram and its quantiles (credible bands of the absorber profile).  Additive: GPDLA_ABI_VERSION is
 * unchanged.  fp64 throughout; tests/absorption_distribution_restatement.py states the same in NumPy.
 *
 * Everything lives on the unmasked-range grid of a selected quasar (n_u pixels, CSR offsets), as for
 * gpdla_batch_model_spectra.
 * Components.  The components m and their per-quasar model weights p_m are those of gpdla_batch_marginal_continuum
 *   (null, the sub-DLA table, the DLA table; model_weights NULL: (0, 0, 1)), for the _multi entry those of
 *   gpdla_batch_marginal_continuum_multi (null, sub-DLA, DLA(1) .. DLA(max_dlas); model_weights NULL: the resident
 *   model_posteriors).  Rows are non-negative, finite, of positive sum, and normalised by their sum.
 * Samples.  Sample i of component m has the broadened profile a_{m,i}(p) of mean_absorption; for DLA(n), n >= 2, the
 *   product of the n gathered profiles in slot order, as mean_absorption_models defines it.  The weights w_{m,i} are
 *   those of mean_absorption: exp(l - max l) / Sum, NaN -> 0.  Write abar = min(max(a, 0), 1).  The null component is
 *   one atom at abar = 1.
 * Exceedance.  F_p(t) = Sum_m p_m Sum_i w_{m,i} [abar_{m,i}(p) <= t].
 * Support.  S_p: the atoms with p_m w_{m,i} > 0, the null atom included when p_null > 0.
 *
 * prob_below [num_thresholds][capacity] = F_p(t_j); the thresholds are finite and strictly inside (0, 1), at most 4.
 *   The null atom never counts (t_j < 1).  The comparison is made on abar itself, not read off the histogram.  The
 *   normalised weights add up to 1 within rounding only: the reported value is min(F, 1).
 * absorption_min, absorption_max [capacity]: the minimum and maximum of abar over S_p.
 * histogram [num_bins][capacity]: H_b(p) = the mass of the atoms with bin(abar) = b,
 *   bin(x) = min(B - 1, (int)(x * (double)B)), B = num_bins in [8, 256]; the null atom falls in bin B - 1.
 * quantiles [num_levels][capacity]: levels l_j strictly inside (0, 1), at most 8.  C_b = H_0 + .. + H_b, added in
 *   ascending b, C_{-1} = 0; b* the first b with C_b >= l (none, by rounding: B - 1);
 *   q = (b* + clamp((l - C_{b*-1}) / H_{b*}, 0, 1)) / B, then clamped to [absorption_min, absorption_max]: an unabsorbed
 *   pixel reports 1, a saturated core 0; elsewhere the error is at most one bin width.  quantiles needs neither of the
 *   other arrays to be requested.
 * num_thresholds = 0: no prob_below.  num_bins = 0: no histogram (num_levels must be 0 then).  Both 0: refused.  A call
 * whose histogram and quantiles pointers are NULL runs the kernel variant without bins whatever num_bins says.
 *
 * Special rows follow the siblings.  A quasar of sweep status 1 or 3 (no kept pixel; unusable noise) gets NaN rows and
 * that status.  A component of positive model weight whose row has no weights gets NaN rows and status 0 (_multi: named in
 * model_flags).  A component of weight exactly 0 is not evaluated; a sample of weight exactly 0 enters nothing.  With
 * GPDLA_SPECTRA_WEIGHTS_REFINED (single-DLA entry only) the DLA component runs on the S' refine points of the quasar's last
 * box, as defined under "THE REFINED SOURCE" above: a selected quasar without a refined table gets NaN rows and
 * GPDLA_SPECTRA_NOT_REFINED, a stale or missing refine pass is GPDLA_ERR_INVALID_ARGUMENT, the sub-DLA component keeps its
 * first-pass table.  A conditioned batch is refused.  weights_source NONE with a null-only mixture is legal: prob_below 0,
 * all mass in bin B - 1, minimum = maximum = quantiles = 1.  _multi: a row of model weights with a NaN gives NaN rows and
 * GPDLA_SPECTRA_AVERAGE_UNDEFINED.
 *
 * Sums run in a fixed order without floating-point atomics (samples in z_DLA order within a wave's 64-sample groups, the
 * groups of a wave in order, the waves in wave order, the components in component order, the null atom last): outputs are
 * bit-identical from run to run, for any selection order and launch grouping, and for the resident and the host form of a
 * table.
 * ------------------------------------------------------------------------------------------- */
#define GPDLA_DISTRIBUTION_MAX_THRESHOLDS 4
#define GPDLA_DISTRIBUTION_MAX_LEVELS 8
#define GPDLA_DISTRIBUTION_MIN_BINS 8
#define GPDLA_DISTRIBUTION_MAX_BINS 256
typedef struct {
  int64_t num_selected;
  const int64_t *selection;          /* [num_selected] quasars of the batch; NULL = 0 .. num_selected-1 */
  int32_t weights_source;            /* GPDLA_SPECTRA_WEIGHTS_RESIDENT, _HOST or _REFINED (_NONE: null component only) */
  const double *sample_log_likelihoods_dla; /* [num_selected][S], _HOST, where a row weighs the DLA table */
  const double *sample_log_likelihoods_lls; /* [num_selected][S], _HOST, where a row weighs the sub-DLA table */
  const double *model_weights;       /* [num_selected][3] (null, sub-DLA, DLA), or NULL = (0, 0, 1) */
  int32_t meanflux;                  /* != 0: the grid of the mean-flux model's prepared rows (the same pixels) */
  int64_t capacity;                  /* entries of each plane of the per-pixel output arrays */
  int32_t num_thresholds;            /* 0 .. 4 */
  const double *thresholds;          /* [num_thresholds], strictly inside (0, 1) */
  int32_t num_bins;                  /* 0, or 8 .. 256 */
  int32_t num_levels;                /* 0 .. 8; > 0 needs num_bins */
  const double *levels;              /* [num_levels], strictly inside (0, 1) */
} gpdla_absorption_distribution_request;
typedef struct {
  int64_t *offsets;                  /* [num_selected + 1]; required */
  double *prob_below;                /* [num_thresholds][capacity] or NULL */
  double *absorption_min, *absorption_max; /* [capacity] or NULL */
  double *histogram;                 /* [num_bins][capacity] or NULL */
  double *quantiles;                 /* [num_levels][capacity] or NULL */
  int32_t *status;                   /* [num_selected] or NULL */
} gpdla_absorption_distribution;
/* The checks of gpdla_marginal_continuum_validate, then this product's: more than 4 thresholds or 8 levels (or a negative
 * count), a count without its array, a threshold or a level that is NaN or not strictly inside (0, 1), num_bins neither 0
 * nor in [8, 256], levels without bins, nothing requested (no thresholds and no bins).  Returns GPDLA_OK or
 * GPDLA_ERR_INVALID_ARGUMENT.  Needs no GPU. */
int gpdla_absorption_distribution_validate(const gpdla_absorption_distribution_request *request, int64_t num_quasars,
                                           int64_t num_samples, int has_lls_nhi_samples);
/* With gpdla_context_set_timing enabled, gpdla_context_last_sweep_ms reports the launch groups of the call:
 * k_absorption_init, per group the staging of a host table's slice, k_spectra_weights and k_absorption_dist per
 * component, and k_absorption_combine. */
int gpdla_batch_absorption_distribution(gpdla_context *ctx, gpdla_batch *batch,
                                        const gpdla_absorption_distribution_request *request,
                                        gpdla_absorption_distribution *out);
typedef struct {
  int64_t num_selected;
  const int64_t *selection;
  int32_t max_dlas;
  int32_t tables_source;
  const double *sample_log_likelihoods_dla;
  const uint32_t *base_sample_inds;
  const double *sample_log_likelihoods_lls;
  const double *model_weights;
  int32_t meanflux;
  int64_t capacity;                  /* the fields of gpdla_marginal_continuum_multi_request up to here */
  int32_t num_thresholds;
  const double *thresholds;
  int32_t num_bins;
  int32_t num_levels;
  const double *levels;
} gpdla_absorption_distribution_multi_request;
typedef struct {
  int64_t *offsets;                  /* [num_selected + 1]; required */
  double *prob_below;
  double *absorption_min, *absorption_max;
  double *histogram;
  double *quantiles;
  int32_t *status;                   /* [num_selected] or NULL */
  uint32_t *model_flags;             /* [num_selected] or NULL */
} gpdla_absorption_distribution_multi;
/* The checks of gpdla_marginal_continuum_multi_validate, then those of gpdla_absorption_distribution_validate. */
int gpdla_absorption_distribution_multi_validate(const gpdla_absorption_distribution_multi_request *request,
                                                 int64_t num_quasars, int64_t num_samples, int has_lls_nhi_samples,
                                                 int batch_max_dlas, int batch_processed);
int gpdla_batch_absorption_distribution_multi(gpdla_context *ctx, gpdla_batch *batch,
                                              const gpdla_absorption_distribution_multi_request *request,
                                              gpdla_absorption_distribution_multi *out);

#ifdef __cplusplus
}
#endif
#endif
