// host_consumers.hpp -- what the entries that read a resident batch after a sweep share (model spectra,
// mock draws, parameter summaries, the refine pass, its download and its summaries): the refusals
// every one of them tests, the resident sample table, the absorber lists and the k_spectra_map launch.
// (Staging and EventPair are in host_common.hpp, begin_timing / end_timing beside gpdla_context in
// host_context.hpp: the sweeps use them too.  What only the per-pixel grid products share -- the selection
// and its offsets, the sample weights, the mixtures' plan -- follows in host_grid.hpp.)
#pragma once

namespace {

// args_ok: the entry's other pointers are not null
int check_batch_pair(const gpdla_context *c, const gpdla_batch *b, bool args_ok = true) {
  if (!c || !b || b->ctx != c || !args_ok) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null/mismatched argument");
  return GPDLA_OK;
}

// selection == nullptr: the first num_selected quasars of the nq
int check_selection(int64_t nq, const int64_t *selection, int64_t num_selected) {
  if (num_selected < 0 || (!selection && num_selected > nq))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "num_selected = %lld outside [0, %lld]", (long long)num_selected, (long long)nq);
  if (selection)
    for (int64_t s = 0; s < num_selected; ++s)
      if (selection[s] < 0 || selection[s] >= nq)
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "selection[%lld] = %lld outside the batch of %lld quasars", (long long)s,
                    (long long)selection[s], (long long)nq);
  return GPDLA_OK;
}

// `what`: printed in front of the refusal ("resident weights: " where only one product needs the sweep)
int check_processed(const gpdla_batch *b, const char *what = "") {
  if (b->md ? (!b->mb || !b->mb->processed) : !b->processed)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "%sthe batch has not been processed", what);
  return GPDLA_OK;
}

// The context still holds what the batch was uploaded for: the number of samples and, model_too, the
// model's rank.  (The entries differ in which they need; each keeps its own.)
int check_unchanged(const gpdla_context *c, const gpdla_batch *b, bool model_too) {
  if (b->S != c->S || (model_too && b->k != c->model.k))
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "%s changed after the batch was uploaded", model_too ? "model/samples" : "samples");
  return GPDLA_OK;
}

// The entries that run k_prepare again (model spectra, mock draws and their hooks) would put unconditioned
// rows where a conditioned batch's refine pass expects its own, and their products are not defined for a
// batch whose results are about "one more absorber" (DESIGN.md 4.20): they refuse it.
int check_unconditioned(const gpdla_batch *b, const char *what) {
  if (b->fx && b->fx->on)
    return fail(GPDLA_ERR_UNSUPPORTED, "%s: the batch is conditioned on fixed absorbers (gpdla_batch_clear_fixed_absorbers first)", what);
  return GPDLA_OK;
}

// The resident sample log-likelihoods of a processed batch: quasar q's row (multi-DLA: its model
// DLA(1) row, [nq][max_dlas][S]; the sub-DLA table is [nq][S]) starts at table + q * width.
struct SampleTable {
  const double *table;
  int64_t width;
};

SampleTable resident_samples(const gpdla_batch *b, bool sub_dla) {
  if (!b->md) return {b->d_sample_ll, b->S};
  return sub_dla ? SampleTable{b->mb->sll_lls, b->S} : SampleTable{b->mb->sll_dla, (int64_t)b->md * b->S};
}

// Absorber lists in CSR form on the device.  The caller's offsets may be a slice of a longer CSR
// (offsets[0] > 0) beside the full z / nhi arrays: the device copy starts at zero.  A host buffer of
// asynchronous copies, so it is declared before the Staging it uploads through.
struct AbsorberLists {
  bool have_abs = false;     // at least one absorber is listed
  std::vector<int64_t> off;  // [n + 1], rebased to zero
  int64_t *d_off = nullptr;  // nullptr unless have_abs or always_offsets
  double *d_z = nullptr, *d_nhi = nullptr;

  int upload(Staging &sg, int64_t n, const int64_t *offsets, const double *z, const double *nhi, bool always_offsets = false) {
    const int64_t a0 = offsets ? offsets[0] : 0, na = offsets ? offsets[n] - a0 : 0;
    have_abs = na > 0;
    if (!have_abs && !always_offsets) return GPDLA_OK;
    off.resize((size_t)n + 1);
    for (int64_t s = 0; s <= n; ++s) off[(size_t)s] = offsets ? offsets[s] - a0 : 0;
    int rc = sg.put(&d_off, off.data(), (size_t)n + 1);
    if (rc || !have_abs) return rc;
    if ((rc = sg.put(&d_z, z + a0, (size_t)na))) return rc;
    return sg.put(&d_nhi, nhi + a0, (size_t)na);
  }
};

// k_spectra_map: the absorption of the listed absorbers on the grids of nsel quasars of the batch
int launch_spectra_map(const gpdla_context *c, const gpdla_batch *b, int64_t nsel, const int64_t *d_sel, const int64_t *d_off,
                       const AbsorberLists &lists, double *d_out, hipStream_t st) {
  SpectraMapArgs ma;
  ma.meta = b->d_meta;
  ma.lam_pad = b->d_lam;
  ma.sel = d_sel;
  ma.abs_off = lists.d_off;
  ma.abs_z = lists.d_z;
  ma.abs_n = lists.d_nhi;
  ma.out_off = d_off;
  ma.num_lines = c->cfg.num_lines;
  ma.out = d_out;
  hipLaunchKernelGGL(k_spectra_map, dim3((unsigned)nsel), dim3(256), 0, st, ma);
  HIP_TRY(hipGetLastError());
  return GPDLA_OK;
}

}  // namespace
