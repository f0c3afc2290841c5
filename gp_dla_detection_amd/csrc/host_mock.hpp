// host_mock.hpp -- mock spectra: one draw per quasar of a resident batch from the
// model the sweeps evaluate, optionally left resident for the next process call.
// Kernels: mock_kernels.hpp (the draw), spectra_kernels.hpp (k_spectra_map: the absorption).
#pragma once

namespace {

int validate_mock(const gpdla_mock_request *rq, int64_t nq) {
  if (!rq) return fail(GPDLA_ERR_INVALID_ARGUMENT, "null request");
  if (nq < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "negative quasar count");
  if (rq->capacity_stored < 0 || rq->capacity_grid < 0) return fail(GPDLA_ERR_INVALID_ARGUMENT, "negative capacity");
  int rc = validate_absorbers(nq, rq->absorber_offsets, rq->absorber_z, rq->absorber_nhi);
  if (rc) return rc;
  if (rq->absorber_offsets)
    for (int64_t j = rq->absorber_offsets[0]; j < rq->absorber_offsets[nq]; ++j) {
      if (!(rq->absorber_nhi[j] > 0.0) || !std::isfinite(rq->absorber_nhi[j]))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "absorber_nhi[%lld] = %g: a column density is finite and positive",
                    (long long)j, rq->absorber_nhi[j]);
      if (!std::isfinite(rq->absorber_z[j]))
        return fail(GPDLA_ERR_INVALID_ARGUMENT, "absorber_z[%lld] = %g is not finite", (long long)j, rq->absorber_z[j]);
    }
  return GPDLA_OK;
}

}  // namespace

extern "C" {

int gpdla_mock_validate(const gpdla_mock_request *rq, int64_t num_quasars) try {
  return validate_mock(rq, num_quasars);
} GPDLA_NO_THROW

int gpdla_batch_draw_mocks(gpdla_context *c, gpdla_batch *b, const gpdla_mock_request *rq, gpdla_mock_spectra *out) try {
  int rc = check_batch_pair(c, b, rq && out && out->grid_offsets);
  if (rc || (rc = check_unconditioned(b, "mock draws")) || (rc = validate_mock(rq, b->nq)) || (rc = check_unchanged(c, b, true))) return rc;
  if (b->k > GPDLA_MAX_K) return fail(GPDLA_ERR_UNSUPPORTED, "k = %d above %d", b->k, GPDLA_MAX_K);
  if (out->flux && rq->capacity_stored < b->total_pix)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the batch stores %lld pixels, capacity_stored is %lld", (long long)b->total_pix,
                (long long)rq->capacity_stored);
  const int64_t nq = b->nq;
  HIP_TRY(hipSetDevice(c->device_id));
  hipStream_t st = c->stream;
  std::vector<QuasarMeta> meta;
  if ((rc = spectra_prepare(c, b, rq->meanflux != 0, meta))) return rc;

  std::vector<int64_t> sel((size_t)nq), off((size_t)nq + 1, 0);
  std::vector<int32_t> status((size_t)nq);
  for (int64_t q = 0; q < nq; ++q) {
    sel[(size_t)q] = q;
    off[(size_t)q + 1] = off[(size_t)q] + meta[(size_t)q].n_u;
    status[(size_t)q] = meta[(size_t)q].status;
  }
  const int64_t total = off[(size_t)nq];
  std::memcpy(out->grid_offsets, off.data(), ((size_t)nq + 1) * sizeof(int64_t));
  if ((out->absorption || out->continuum || out->sigma) && total > rq->capacity_grid)
    return fail(GPDLA_ERR_INVALID_ARGUMENT, "the batch has %lld grid pixels, capacity_grid is %lld (grid_offsets are written)",
                (long long)total, (long long)rq->capacity_grid);
  if (out->status) std::memcpy(out->status, status.data(), (size_t)nq * sizeof(int32_t));
  if (nq == 0) return GPDLA_OK;

  AbsorberLists lists;
  Staging sg(st);
  int64_t *d_sel = nullptr, *d_off = nullptr;
  if ((rc = sg.put(&d_off, off.data(), (size_t)nq + 1))) return rc;
  if ((rc = lists.upload(sg, nq, rq->absorber_offsets, rq->absorber_z, rq->absorber_nhi))) return rc;
  const size_t tot = (size_t)total, npx = (size_t)b->total_pix;

  // a: k_spectra_map over the whole batch (skipped when it would be all ones and nobody asked for it)
  double *d_abs = nullptr;
  if (lists.have_abs || out->absorption) {
    if ((rc = sg.put(&d_sel, sel.data(), (size_t)nq)) || (rc = sg.tmp.alloc(&d_abs, tot))) return rc;
    if ((rc = launch_spectra_map(c, b, nq, d_sel, d_off, lists, d_abs, st))) return rc;
  }

  double *d_flux = b->d_flux, *d_cont = nullptr, *d_sig = nullptr, *d_lat = nullptr;
  if (!rq->write_resident) {  // the draw is in place: on a copy of the resident flux
    if ((rc = sg.tmp.alloc(&d_flux, npx))) return rc;
    if (npx) HIP_TRY(hipMemcpyAsync(d_flux, b->d_flux, npx * sizeof(double), hipMemcpyDeviceToDevice, st));
  }
  if (out->continuum && (rc = sg.tmp.alloc(&d_cont, tot))) return rc;
  if (out->sigma && (rc = sg.tmp.alloc(&d_sig, tot))) return rc;
  if (out->latents && (rc = sg.tmp.alloc(&d_lat, (size_t)nq * (size_t)b->k))) return rc;
  MockDrawArgs da;
  da.meta = b->d_meta;
  da.pix = b->d_pix;
  da.Mi = b->d_Mi;
  da.offsets = b->d_offsets;
  da.wavelengths = b->d_wl;
  da.noise_variance = b->d_nv;
  da.pixel_mask = b->d_mask;
  da.z_qsos = b->d_z;
  da.min_lambda = c->cfg.min_lambda;
  da.max_lambda = c->cfg.max_lambda;
  da.k = b->k;
  da.seed = rq->seed;
  da.first_quasar_index = c->cfg.first_quasar_index;
  da.grid_off = d_off;
  da.absorption = lists.have_abs ? d_abs : nullptr;
  da.flux = d_flux;
  da.continuum = d_cont;
  da.sigma = d_sig;
  da.latents = d_lat;
  if (rq->write_resident) {  // whatever was computed from the previous flux is stale from here on
    b->processed = false;
    if (b->mb) b->mb->processed = false;
  }
  if ((rc = begin_timing(c, st))) return rc;
  hipLaunchKernelGGL(k_mock_draw, dim3((unsigned)nq), dim3(256), 0, st, da);
  HIP_TRY(hipGetLastError());
  if ((rc = end_timing(c, st))) return rc;
  if ((rc = sg.fetch(out->flux, d_flux, npx)) || (rc = sg.fetch(out->absorption, d_abs, tot)) ||
      (rc = sg.fetch(out->continuum, d_cont, tot)) || (rc = sg.fetch(out->sigma, d_sig, tot)) ||
      (rc = sg.fetch(out->latents, d_lat, (size_t)nq * (size_t)b->k)))
    return rc;
  HIP_TRY(hipStreamSynchronize(st));
  return GPDLA_OK;
} GPDLA_NO_THROW

}  // extern "C"
